"""Helpers of tests/test_stream_cpu.py and tests/test_stream_gpu.py: the three streaming families side by side (engine
constructors, parameters with batch-norm rows drawn at random per timestep, the float64 reference over a concatenated stream),
a driver that cuts a stream into forward_stream calls, and a fake model for the host-only tests of stream.GazeStream."""
import numpy as np
import torch

from recurrent_gaze_prediction_amd import synthetic as syn

FAMILIES = ('grcn', 'grcn77', 'lstm')
PLANS = [('f32', False), ('bf16', False), ('bf16', True)]        # (dtype, per_step): f32 per-step, bf16 persistent, bf16 per-step
PLAN_IDS = ['f32', 'bf16-persistent', 'bf16-per_step']
STATE_PARTS = {'grcn': 1, 'grcn77': 1, 'lstm': 2}
MAP_HW = {'grcn': 49, 'grcn77': 7, 'lstm': 49}


def params(family, T):
    """Parameters of a T-step plan.  gaze_grcn's batch-norm gamma / beta are random per timestep (with the identity a wrong
    phase is invisible); the other two graphs have no per-timestep variable."""
    if family == 'grcn':
        return syn.grcn_params(71, T, gru_std=0.05, random_bn=True)
    if family == 'grcn77':
        return syn.grcn77_params(72)
    return syn.lstm_params(73)


def tile_bn(p, T_long):
    """The parameters of a T_long-step gaze_grcn plan whose step s uses batch-norm row s % T of p."""
    q = dict(p)
    idx = np.arange(T_long) % len(p['bn_gamma'])
    q['bn_gamma'], q['bn_beta'] = np.asarray(p['bn_gamma'])[idx], np.asarray(p['bn_beta'])[idx]
    return q


def engine(family, B, T, dtype, per_step, gpu, p=None, save=False):
    """The family's engine on the named path: bf16 not per_step must be the persistent kernel."""
    from recurrent_gaze_prediction_amd import engine as E
    if family == 'grcn':
        eng = E.GrcnEngine(B, T, dtype=dtype, device=gpu, per_step=per_step, save_for_backward=save)
    elif family == 'grcn77':
        eng = E.Grcn77Engine(B, T, dtype=dtype, device=gpu, per_step=per_step, save_for_backward=save)
    else:
        eng = E.LstmEngine(B, T, dtype=dtype, device=gpu, per_step=per_step, persistent=(dtype == 'bf16' and not per_step),
                           save_for_backward=save)
    assert eng.persistent == (dtype == 'bf16' and not per_step)
    if p is not None:
        eng.set_weights(p)
    return eng


def last_state(family, eng, B, T):
    """The state behind step T of the plan's last forward, from read_buffer, in forward_stream's layout (flat)."""
    if family == 'lstm':
        parts = [eng.read_buffer(k).reshape(B, T, 49 * 128)[:, -1] for k in ('h', 'c')]
        return torch.stack(parts).reshape(-1)
    return eng.read_buffer('rcn_outputs').reshape(B, T, -1)[:, -1].reshape(-1)


def run_stream(family, eng, x, cuts, pad_value=0.0, use_rows=None, probs_out=None):
    """x [B, N, 1024, 7, 7] device tensor; cuts: steps per call (each <= T, sum N).  Calls forward_stream once per cut with the
    chunk padded to T steps by pad_value (those steps lie behind n_valid: they must not matter) and, for gaze_grcn, the
    batch-norm phase of the stream position.  -> (logits [B, N, H, W], final state); the softmax maps of each call's valid steps are
    appended to probs_out if it is a list."""
    B, T = eng.B, eng.T
    assert sum(cuts) == x.shape[1]
    state, pos, out = None, 0, []
    for n in cuts:
        chunk = torch.full((B, T, 1024, 7, 7), float(pad_value), device=x.device)
        chunk[:, :n] = x[:, pos:pos + n]
        kw = {'bn_phase': pos % T} if family == 'grcn' else {}
        if use_rows is not None:
            logits, probs, new_state = eng.forward_stream(rows=use_rows(chunk), state=state, n_valid=n, **kw)
        else:
            logits, probs, new_state = eng.forward_stream(chunk, state=state, n_valid=n, **kw)
        if probs_out is not None:
            probs_out.append(probs[:, :n].clone())
        assert state is None or new_state.data_ptr() != state.data_ptr()
        out.append(logits[:, :n].clone())
        state, pos = new_state, pos + n
    return torch.cat(out, 1), state


def to_rows(xd, dtype):
    """[B,T,1024,7,7] (channel c*2+d) -> conv5b rows [B*T*49, 1024] with column d*512+c, as C3DEngine writes them."""
    td = torch.bfloat16 if dtype == 'bf16' else torch.float32
    return xd.permute(0, 1, 3, 4, 2).reshape(-1, 512, 2).transpose(1, 2).reshape(-1, 1024).contiguous().to(td)


def reference_f64(family, x, p, T, emulate_bf16=False):
    """float64 over the whole stream x [B, N, ...] as ONE recurrence from zeros (gaze_grcn: batch-norm row s % T at step s)
    -> (logits [B,N,H,W], {'h': [B,N,7,7,128] (, 'c')}) as numpy."""
    N = x.shape[1]
    if family == 'grcn':
        from oracle import torch_ref
        pt = {k: torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in tile_bn(p, N).items()}
        logits, hs, _ = torch_ref.grcn_forward(torch.tensor(x, dtype=torch.float64), pt, want_hidden=True)
        return logits.numpy(), {'h': hs.numpy()}
    if family == 'grcn77':
        import grcn77_ref
        z, h, _ = grcn77_ref.forward_f64(x, p)
        return z, {'h': h}
    import lstm_ref
    pt = lstm_ref._params(p)
    with torch.no_grad():
        logits, it = lstm_ref.lstm_forward(torch.as_tensor(np.asarray(x), dtype=torch.float64), pt, True, emulate_bf16)
    return logits.numpy(), {'h': it['h'].numpy(), 'c': it['c'].numpy()}


def state_parts(family, state, B):
    """flat device state -> {'h': [B,7,7,128] (, 'c')} numpy"""
    s = state.detach().cpu().numpy().reshape(STATE_PARTS[family], B, 7, 7, 128)
    return {'h': s[0], 'c': s[1]} if family == 'lstm' else {'h': s[0]}


# ---------------------------------------------------------------------------------------------- host-only fake model
class FakeStreamModel(object):
    """predict_stream keeps a running sum of its inputs per lane and honours n_valid: the map of step t is the sum of the lane's
    feature [.., 0, 0, 0] over the steps since its last reset, broadcast over a 2 x 2 map.  Records its calls."""
    gazemap_height = gazemap_width = 2
    STATE_PARTS = 1

    def __init__(self, B, T):
        self.batch_size, self.n_lstm_steps = B, T
        self.stream_calls, self.predict_calls = [], []

    def predict_stream(self, c3d, state=None, n_valid=None, position=0):
        x = torch.as_tensor(np.asarray(c3d)).reshape(self.batch_size, self.n_lstm_steps, 1024, 7, 7)[:, :, 0, 0, 0].double()
        n_valid = self.n_lstm_steps if n_valid is None else n_valid
        s0 = torch.zeros(self.batch_size, dtype=torch.float64) if state is None else state
        before = s0.clone()
        sums = s0[:, None] + torch.cumsum(x, 1)
        maps = sums[:, :, None, None].expand(-1, -1, 2, 2).clone()
        maps[:, n_valid:] = float('nan')                       # unspecified behind n_valid
        new_state = sums[:, n_valid - 1].clone()
        assert torch.equal(s0, before)
        self.stream_calls.append((n_valid, position, None if state is None else state.clone()))
        return maps, new_state

    def predict(self, c3d, frames=None):
        x = np.asarray(c3d)
        self.predict_calls.append(x.copy())
        s = np.cumsum(x.reshape(self.batch_size, self.n_lstm_steps, 1024, 7, 7)[:, :, 0, 0, 0].astype(np.float64), 1)
        return torch.tensor(np.broadcast_to(s[:, :, None, None], s.shape + (2, 2)).copy())


def fake_clip(seed, n):
    """[n, 1024, 7, 7] features whose element [t, 0, 0, 0] is a small integer (sums are exact)."""
    rs = np.random.RandomState(seed)
    c = np.zeros((n, 1024, 7, 7), np.float32)
    c[:, 0, 0, 0] = rs.randint(1, 50, n)
    return c
