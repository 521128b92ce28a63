"""Helpers of tests/test_cascade_stream_cpu.py and tests/test_cascade_stream_gpu.py: the float64 cascade with initial states
(the loop of torch_ref.cascade_forward, started from h0 / g0 instead of zeros), inputs as tests/test_cascade_gpu.run_case
draws them, a driver that cuts a stream into forward_stream calls, the state's two halves, and a fake model with a
two-part state that records the frames it is handed (host-only tests of stream.GazeStream)."""
import functools

import numpy as np
import torch

from oracle import torch_ref
from recurrent_gaze_prediction_amd import synthetic as syn

BOT, TOP = 49 * 256, 2401 * 3                     # per-lane fp32 elements of the two parts of a state
SEEDS = (301, 411)


def to_t(p, dtype=torch.float64):
    return {k: to_t(v, dtype) if isinstance(v, dict) else torch.tensor(v, dtype=dtype) for k, v in p.items()}


def rel_err(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30))


def inputs(seed, B, N):
    """frames [B,N,98,98,3], c3d [B,N,1024,7,7] fp32, as run_case(gpu, dtype, B, N, seed) makes them."""
    rs = np.random.RandomState(seed + 7)
    frames = rs.rand(B, N, 98, 98, 3).astype(np.float32)
    return frames, syn.c3d_features(seed + 8, B, N)


def cascade_forward_from(frame_images, c3d_input, p, h0=None, g0=None):
    """torch_ref.cascade_forward (dropout off) with the bottom state h0 [B,7,7,256] and the top state g0 [B,49,49,3] it starts
    from (None: zeros) -> (maps [B,T,49,49], bottom states [B,T,7,7,256], top states [B,T,49,49,3])."""
    b, t = c3d_input.shape[:2]
    sal = torch_ref.shallownet_forward(frame_images.reshape((-1,) + tuple(frame_images.shape[2:])), p['ShallowNet'])
    sal = sal.reshape(b, t, 49, 49, 1)
    xr = c3d_input.permute(0, 1, 3, 4, 2)
    emb = (xr.reshape(-1, 1024) @ p['proj_c3d_W'] + p['proj_c3d_b']).reshape(b, t, 7, 7, -1)
    bot = {k[len('RCNBottom/'):]: v for k, v in p.items() if k.startswith('RCNBottom/')}
    top = {k[len('RCNGaze/'):]: v for k, v in p.items() if k.startswith('RCNGaze/')}
    h = torch.zeros(b, 7, 7, bot['GRU_Conv_Uz'].shape[-1], dtype=c3d_input.dtype) if h0 is None else h0
    g = torch.zeros(b, 49, 49, top['GRU_Conv_Uz'].shape[-1], dtype=c3d_input.dtype) if g0 is None else g0
    outs, hs, gs = [], [], []
    for i in range(t):
        h = torch_ref.grcn_cell(emb[:, i], h, bot)
        up = torch_ref.conv2d_transpose(h, p['Upsampling/weight'], 7, 'SAME')
        g = torch_ref.grcn_cell(torch.cat([up, sal[:, i]], -1), g, top)
        x = g.reshape(b, -1)
        x = torch.relu(x @ p['LastProjection/fc1_w'] + p['LastProjection/fc1_b'])
        x = torch.maximum(x[:, :2401], x[:, 2401:])
        x = torch.relu(x @ p['LastProjection/fc2_w'] + p['LastProjection/fc2_b'])
        x = torch.maximum(x[:, :2401], x[:, 2401:])
        outs.append(x.reshape(b, 49, 49))
        hs.append(h)
        gs.append(g)
    return torch.stack(outs, 1), torch.stack(hs, 1), torch.stack(gs, 1)


@functools.lru_cache(maxsize=None)
def stream_reference(seed, B=2, N=7):
    """The N-step stream of `seed` as ONE float64 recurrence from zeros, computed once and shared (do not modify):
    (params, frames, c3d, maps [B,N,49,49], bottom [B,N,7,7,256], top [B,N,49,49,3]), the last three numpy float64."""
    p = syn.cascade_params(seed)
    frames, c3d = inputs(seed, B, N)
    with torch.no_grad():
        maps, hs, gs = cascade_forward_from(torch.tensor(frames, dtype=torch.float64), torch.tensor(c3d, dtype=torch.float64), to_t(p))
    return p, frames, c3d, maps.numpy(), hs.numpy(), gs.numpy()


def split_state(state, B):
    """flat state -> (bottom [B, 49*256], top [B, 2401*3]) views"""
    s = state.reshape(-1)
    assert s.numel() == B * (BOT + TOP)
    return s[:B * BOT].view(B, BOT), s[B * BOT:].view(B, TOP)


def run_stream(eng, frames, c3d, cuts, pad_value=0.0, carry='both'):
    """frames [B,N,98,98,3], c3d [B,N,1024,7,7] device tensors; cuts: steps per call (each <= T, sum N).  One forward_stream per
    cut, the chunk padded to T steps by pad_value -- features AND frames; those steps lie behind n_valid and must not matter.
    carry: 'both' hands every new state on as it is, 'none' passes state=None every time, 'bottom' / 'top' zero the other half
    of the carried state.  -> (maps [B,N,49,49], final state)."""
    B, T = eng.batch, eng.n_steps
    assert sum(cuts) == c3d.shape[1] == frames.shape[1]
    state, pos, out = None, 0, []
    for n in cuts:
        x = torch.full((B, T, 1024, 7, 7), float(pad_value), device=c3d.device)
        f = torch.full((B, T) + tuple(frames.shape[2:]), float(pad_value), device=c3d.device)
        x[:, :n], f[:, :n] = c3d[:, pos:pos + n], frames[:, pos:pos + n]
        maps, new_state = eng.forward_stream(f, x, state=state, n_valid=n)
        assert state is None or new_state.data_ptr() != state.data_ptr()
        out.append(maps[:, :n].clone())
        pos += n
        if carry == 'none':
            state = None
        else:
            state = new_state
            if carry != 'both':
                state = new_state.clone()
                bot, top = split_state(state, B)
                (top if carry == 'bottom' else bot).zero_()
    return torch.cat(out, 1), state


# ---------------------------------------------------------------------------------------------- host-only fake model
class FakeFramesModel(object):
    """A model with a two-part state of per-lane sizes (3, 5) that takes frames: part 0 of a lane holds the running sum of its
    feature [.., 0, 0, 0], part 1 the running sum of its frames' pixel [.., 0, 0, 0]; the map of a step is the sum of the two,
    broadcast over a 2 x 2 map.  Records what it is handed."""
    gazemap_height = gazemap_width = 2
    STATE_LANE_ELEMS = (3, 5)
    NEEDS_FRAMES = True

    def __init__(self, B, T, hw=2):
        self.batch_size, self.n_lstm_steps, self.hw = B, T, hw
        self.stream_calls = []          # (n_valid, position, state or None, frames [B,T,hw,hw,3] numpy)

    def predict_stream(self, c3d, state=None, n_valid=None, position=0, frames=None):
        B, T = self.batch_size, self.n_lstm_steps
        if frames is None:
            raise ValueError('frames')
        x = torch.as_tensor(np.asarray(c3d)).reshape(B, T, 1024, 7, 7)[:, :, 0, 0, 0].double()
        f = torch.as_tensor(np.asarray(frames)).reshape(B, T, self.hw, self.hw, 3)
        n_valid = T if n_valid is None else n_valid
        s0 = torch.zeros(B * 8, dtype=torch.float64) if state is None else state
        before = s0.clone()
        sx = s0[:B * 3].view(B, 3)[:, :1] + torch.cumsum(x, 1)
        sf = s0[B * 3:].view(B, 5)[:, :1] + torch.cumsum(f[:, :, 0, 0, 0].double(), 1)
        maps = (sx + sf)[:, :, None, None].expand(-1, -1, 2, 2).clone()
        maps[:, n_valid:] = float('nan')
        new_state = torch.cat([sx[:, n_valid - 1, None].expand(B, 3).reshape(-1), sf[:, n_valid - 1, None].expand(B, 5).reshape(-1)])
        assert torch.equal(s0, before)
        self.stream_calls.append((n_valid, position, None if state is None else state.clone(), f.numpy().copy()))
        return maps, new_state


def fake_frames(seed, n, hw=2):
    """[n, hw, hw, 3] images whose pixel [t, 0, 0, 0] is a small integer (sums are exact) and the rest a tag of t."""
    rs = np.random.RandomState(seed)
    f = np.zeros((n, hw, hw, 3), np.float32)
    f[:, 0, 0, 0] = rs.randint(1, 50, n)
    f[:, 1, 1, 2] = 1000 * seed + np.arange(n)
    return f
