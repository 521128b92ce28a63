"""torch-CPU restatement of gaze_c3d_conv, the no-recurrence baseline (test helper, built from the oracle's operators).

Reference lines followed: /root/reference/models/gaze_c3d_conv.py
  projection                :116-138   (both tf.nn.dropout sites :132-133, :207 are inert, as SURVEY 9-Q2 describes)
  the three transposed convs :179-204  (tf.concat of one tensor :192 is the identity)
  out_W / out_b             :206-209
softmax and loss are GazePredictionGRU's (gaze_rnn.py:149-159, 363-408): oracle.torch_ref.softmax_maps / gaze_loss.
"""
import numpy as np
import torch

from oracle.torch_ref import conv2d_transpose, gaze_loss, softmax_maps  # noqa: F401

KEYS = ('proj_c3d_W', 'proj_c3d_b', 'weight1', 'weight2', 'weight3', 'out_W', 'out_b')


def c3d_conv_forward(c3d_input, p, want_embedded=False):
    """c3d_input [B,T,1024,7,7], p keyed by KEYS -> logits [B,T,49,49]."""
    b, t = c3d_input.shape[:2]
    xr = c3d_input.permute(0, 1, 3, 4, 2)
    emb = (xr.reshape(-1, 1024) @ p['proj_c3d_W'] + p['proj_c3d_b']).reshape(b * t, 7, 7, -1)
    y = conv2d_transpose(emb, p['weight1'], 3, 'VALID')
    y = conv2d_transpose(y, p['weight2'], 2, 'VALID')
    y = conv2d_transpose(y, p['weight3'], 1, 'SAME')
    z = y.reshape(-1, y.shape[-1]) @ p['out_W'] + p['out_b']
    logits = z.reshape(b, t, 49, 49)
    return (logits, emb) if want_embedded else logits


def forward_f64(x, params):
    """numpy in, numpy float64 logits out."""
    p = {k: torch.as_tensor(np.asarray(params[k]), dtype=torch.float64) for k in KEYS}
    return c3d_conv_forward(torch.as_tensor(np.asarray(x), dtype=torch.float64), p).numpy()


def loss_and_grads(x, gt, params, loss_type='xentropy', want_input_grad=False):
    """loss + d loss / d params (and d loss / d c3d_input) by float64 autograd."""
    p = {k: torch.as_tensor(np.asarray(params[k]), dtype=torch.float64).clone().requires_grad_(True) for k in KEYS}
    xt = torch.as_tensor(np.asarray(x), dtype=torch.float64).clone().requires_grad_(want_input_grad)
    logits = c3d_conv_forward(xt, p)
    ls = gaze_loss(logits, torch.as_tensor(np.asarray(gt), dtype=torch.float64), loss_type)
    ls.backward()
    grads = {k: v.grad.detach().numpy() for k, v in p.items()}
    if want_input_grad:
        grads['c3d_input'] = xt.grad.detach().numpy()
    return ls.item(), logits.detach().numpy(), grads


# ---- the fold, restated in numpy from the formulas of csrc/head_fold.hip.h and csrc/c3dconv_fused.hip.h (float64) ----
def fold_numpy(params):
    """-> (M2 [361, 1024], plane [49, 49]) with logit[f,y,x] = plane[y,x] + sum_{m,n} (X_f[m,n] . M2[(y-6m+3)*19 + x-6n+3])."""
    w = {k: np.asarray(params[k], np.float64) for k in KEYS}
    g = np.einsum('aboc,o->abc', w['weight3'], w['out_W'][:, 0])                     # G[a,b,c]       7 x 7 x 32
    h = np.zeros((11, 11, 64))                                                       # H[p+3,q+3,k]
    for a in range(7):
        for a1 in range(5):
            for b in range(7):
                for b1 in range(5):
                    h[a1 + a, b1 + b] += np.einsum('c,ck->k', g[a, b], w['weight2'][a1, b1])
    s = w['weight1'].shape[-1]
    k = np.zeros((19, 19, s))                                                        # K[r+3,t+3,s]
    for a in range(5):
        for b in range(5):
            k[2 * a:2 * a + 11, 2 * b:2 * b + 11] += np.einsum('pqk,ks->pqs', h, w['weight1'][a, b])
    kf = k.reshape(361, s)
    m2 = kf @ w['proj_c3d_W'].T                                                      # [361, 1024]
    beta = (kf @ w['proj_c3d_b']).reshape(19, 19)
    plane = np.full((49, 49), w['out_b'][0])
    for m in range(7):
        for n in range(7):
            y0, x0 = 6 * m - 3, 6 * n - 3
            ys, xs = slice(max(y0, 0), min(y0 + 19, 49)), slice(max(x0, 0), min(x0 + 19, 49))
            plane[ys, xs] += beta[ys.start - y0:ys.stop - y0, xs.start - x0:xs.stop - x0]
    return m2, plane


def folded_forward_numpy(x, params):
    """The folded network on c3d_input [B,T,1024,7,7] (float64): Z = X M2^T, col2im, + plane."""
    m2, plane = fold_numpy(params)
    x = np.asarray(x, np.float64)
    b, t = x.shape[:2]
    rows = x.transpose(0, 1, 3, 4, 2).reshape(b * t, 7, 7, 1024)
    z = (rows @ m2.T).reshape(b * t, 7, 7, 19, 19)
    out = np.broadcast_to(plane, (b * t, 49, 49)).copy()
    for m in range(7):
        for n in range(7):
            y0, x0 = 6 * m - 3, 6 * n - 3
            ys, xs = slice(max(y0, 0), min(y0 + 19, 49)), slice(max(x0, 0), min(x0 + 19, 49))
            out[:, ys, xs] += z[:, m, n, ys.start - y0:ys.stop - y0, xs.start - x0:xs.stop - x0]
    return out.reshape(b, t, 49, 49)
