"""Streaming gaze prediction: a recurrent model of the family (the conv-recurrent ones, the cascade and the fc-GRU models
gaze_rnn / gaze_rnn77) run on a video longer than its plan as ONE recurrence, the state carried from call to call
(engine.forward_stream, include/rgp.h rgp_*_forward_stream), instead of the reference's T-step chunks that each start from
zeros (extract_map.py:65; SURVEY "State is not carried between chunks")."""
import numpy as np
import torch


class GazeStream(object):
    """B lanes, one clip per lane, all at the same stream position.

    model: GazePredictionGRCN / GazePredictionGRCN77 / GazePredictionLSTM / the cascade's GazePredictionGRCN / the fc-GRU
    GazePredictionGRU of gaze_rnn and gaze_rnn77, whose state is one [B, 1617] part (anything
    with predict_stream, batch_size, n_lstm_steps; the cascade also takes the steps' frame images).  c3d_engine: a C3DEngine of the model's operand dtype for push_windows.
    `position` is the stream position of the next step; gaze_grcn's per-timestep batch-norm slot is position % T, so the
    maps do not depend on how the stream is cut into calls."""

    def __init__(self, model, c3d_engine=None):
        self.model, self.c3d_engine = model, c3d_engine
        self.B, self.T = model.batch_size, model.n_lstm_steps
        self.state = None            # None = the zero state
        self.position = 0

    def reset(self, lanes=None):
        """Zero the state of `lanes` (default: all, which also rewinds `position` to 0).  A lane reset while position % T != 0
        starts its clip in a later batch-norm slot than slot 0 (gaze_grcn): reset at multiples of T for the reference's slots."""
        if lanes is None:
            self.state, self.position = None, 0
            return
        if self.state is not None:
            s = self.state.clone()                                      # states handed out earlier stay as they were
            sizes = getattr(self.model, 'STATE_LANE_ELEMS', None)
            if sizes is None:                                           # equal parts: [parts, B, -1]
                s.view(getattr(self.model, 'STATE_PARTS', 1), self.B, -1)[:, list(lanes)] = 0
            else:                                                       # parts of different per-lane sizes, one after the other
                off = 0
                for n in sizes:
                    s.view(-1)[off:off + self.B * n].view(self.B, n)[list(lanes)] = 0
                    off += self.B * n
                assert off == s.numel(), (off, s.numel())
            self.state = s

    def _advance(self, maps, new_state, n, n_valid):
        self.state = new_state
        self.position += n_valid
        return maps[:, :n]

    def push_features(self, c3d, n_valid=None, frames=None):
        """c3d [B, n <= T, 1024, 7, 7] C3D features of the next n steps of every lane -> maps [B, n, GH, GW].  The
        state advances by n_valid (default n) steps; maps behind step n_valid are unspecified.  frames [B, n, hw, hw, 3]: the
        frame images of the same steps, zero-padded to T beside the features and handed to the models that declare NEEDS_FRAMES
        (the cascade); for every other model they are accepted and ignored, as predict(c3d, frames) ignores them."""
        x = c3d if torch.is_tensor(c3d) else torch.as_tensor(np.asarray(c3d, np.float32))
        x = x.reshape(self.B, -1, 1024, 7, 7)
        n = x.shape[1]
        assert 1 <= n <= self.T, 'push at most T = %d steps per call, got %d' % (self.T, n)
        n_valid = n if n_valid is None else int(n_valid)
        assert 1 <= n_valid <= n, n_valid
        if n < self.T:
            x = torch.cat([x, x.new_zeros((self.B, self.T - n) + tuple(x.shape[2:]))], 1)
        kw = {}
        if frames is not None and getattr(self.model, 'NEEDS_FRAMES', False):
            f = frames if torch.is_tensor(frames) else torch.as_tensor(np.asarray(frames, np.float32))
            assert f.shape[0] == self.B and f.shape[1] == n and f.dim() == 5, (tuple(f.shape), self.B, n)
            if n < self.T:
                f = torch.cat([f, f.new_zeros((self.B, self.T - n) + tuple(f.shape[2:]))], 1)
            kw['frames'] = f
        maps, new_state = self.model.predict_stream(x, state=self.state, n_valid=n_valid, position=self.position, **kw)
        return self._advance(maps, new_state, n, n_valid)

    def push_windows(self, video, n_valid=None, frame_images=None):
        """video [B*T, 16, 112, 112, 3] fp32 device tensor (window b*T + t = step t of lane b, the full plan size) -> maps
        [B, T, GH, GW].  C3D conv5b rows go straight into the recurrent engine (C3DEngine.forward(want_rows=True), the rows
        variant of forward_stream): frames to maps without leaving the device.  A model whose engine has no rows entry (the
        cascade, the fc-GRU models) gets the C3D features instead, through predict_stream with frame_images [B, T, hw, hw, 3]."""
        assert self.c3d_engine is not None, 'GazeStream(model, c3d_engine=...) for push_windows'
        model, T = self.model, self.T
        n_valid = T if n_valid is None else int(n_valid)
        if not hasattr(model.engine, 'forward_rows'):
            feats = self.c3d_engine.forward(video, want_features=True)[0]
            return self.push_features(feats.reshape(self.B, T, 1024, 7, 7), n_valid=n_valid, frames=frame_images)
        rows = self.c3d_engine.forward(video, want_features=False, want_rows=True)[1]
        want_probs = model.config.loss_type in ('xentropy', 'KLD')

        def run():
            kw = {'bn_phase': self.position % T} if model.engine.STREAM_BN_PHASE else {}
            return model.engine.forward_stream(rows=rows, state=self.state, n_valid=n_valid, want_probs=want_probs, **kw)
        logits, probs, new_state = run()
        if model._status_or_recover():
            logits, probs, new_state = run()
            model._status_or_recover(final=True)
        return self._advance(probs if want_probs else logits, new_state, T, n_valid)


def _host_f32(a):
    return a.detach().to('cpu', torch.float32).numpy() if torch.is_tensor(a) else np.asarray(a, np.float32)


def predict_long_clips(model, clips, frames=None):
    """clips: a list of C3D feature arrays [N_i, 1024, 7, 7] of any lengths -> a list of maps [N_i, GH, GW] (numpy), each
    clip one recurrence from the zero state.  B lanes, T steps per call; a lane that finishes its clip takes the next one
    with a zeroed state at the next call boundary, so every clip starts at batch-norm slot 0 (the calls are whole: all
    lanes share position % T == 0); tails are zero-padded and trimmed.  frames: a list parallel to clips of frame images
    [N_i, hw, hw, 3], cut, padded and trimmed like the features.  The models that declare NEEDS_FRAMES (the cascade) require
    them (ValueError without); for every other model they are ignored, whatever they are, and nothing is passed on."""
    stream = GazeStream(model)
    B, T = stream.B, stream.T
    clips = [np.asarray(c, np.float32).reshape(len(c), 1024, 7, 7) for c in clips]
    if not getattr(model, 'NEEDS_FRAMES', False):
        frames = None
    elif frames is None:
        raise ValueError('predict_long_clips: %s needs the frame images of every clip (frames=[...])' % type(model).__name__)
    img_shape = ()
    if frames is not None:
        frames = [_host_f32(f) for f in frames]
        assert len(frames) == len(clips) and all(len(f) == len(c) for f, c in zip(frames, clips)), \
            'frames parallel to clips: one [N_i, hw, hw, 3] array per clip, N_i the clip\'s steps'
        img_shape = next((tuple(f.shape[1:]) for f in frames if len(f)), ())
        assert all(tuple(f.shape[1:]) == img_shape for f in frames if len(f)) and (not img_shape or len(img_shape) == 3), \
            'frames: every clip\'s images share one [hw, hw, 3] shape, got %s' % sorted({tuple(f.shape[1:]) for f in frames if len(f)})
    outs = [[] for _ in clips]
    lane_clip, lane_pos = [None] * B, [0] * B
    nxt = 0
    while True:
        fresh = []
        for b in range(B):
            if lane_clip[b] is not None and lane_pos[b] >= len(clips[lane_clip[b]]):
                lane_clip[b] = None
            while lane_clip[b] is None and nxt < len(clips):
                if len(clips[nxt]):
                    lane_clip[b], lane_pos[b] = nxt, 0
                    fresh.append(b)
                nxt += 1
        if all(c is None for c in lane_clip):
            break
        if fresh:
            stream.reset(fresh)
        x = np.zeros((B, T, 1024, 7, 7), np.float32)
        f = np.zeros((B, T) + img_shape, np.float32) if frames is not None else None
        for b in range(B):
            if lane_clip[b] is not None:
                part = clips[lane_clip[b]][lane_pos[b]:lane_pos[b] + T]
                x[b, :len(part)] = part
                if f is not None:
                    f[b, :len(part)] = frames[lane_clip[b]][lane_pos[b]:lane_pos[b] + T]
        maps = stream.push_features(x) if f is None else stream.push_features(x, frames=f)
        maps = maps.detach().cpu().numpy() if torch.is_tensor(maps) else np.asarray(maps)
        for b in range(B):
            if lane_clip[b] is not None:
                k = min(T, len(clips[lane_clip[b]]) - lane_pos[b])
                outs[lane_clip[b]].append(maps[b, :k].copy())
                lane_pos[b] += T
    gh_gw = (getattr(model, 'gazemap_height', 0), getattr(model, 'gazemap_width', 0))
    return [np.concatenate(o) if o else np.zeros((0,) + gh_gw, np.float32) for o in outs]


def train_long_clips(model, clips, gazemaps, mode='truncated'):
    """Training beside predict_long_clips (the fc-GRU models and gaze_grcn): B clips of ONE length S, C3D features [S, 1024, 7, 7] and gaze
    maps [S, GH, GW] each, one per lane -> model.train_long_clip on the stacked film: every clip one recurrence from the zero
    state, cut into the plan's T-step chunks.  Returns the mean loss."""
    assert len(clips) == len(gazemaps) == model.batch_size, 'one clip and one map array per lane (%d)' % model.batch_size
    x = np.stack([_host_f32(c).reshape(-1, 1024, 7, 7) for c in clips])
    g = np.stack([_host_f32(m) for m in gazemaps])
    assert x.shape[1] == g.shape[1], 'clips and gazemaps of one length, got %d and %d steps' % (x.shape[1], g.shape[1])
    return model.train_long_clip(x, g, mode=mode)


def predict_video(model, frames_u8, extractor, image_hw=98):
    """One uint8 clip [N, H, W, 3] -> maps [n_windows, GH, GW] (numpy) as ONE recurrence: frames.video_inputs makes the C3D
    features of the windows and the frame image paired with each on the device, predict_long_clips streams them and hands
    the images only to the models that take them (the cascade)."""
    from .frames import video_inputs
    _, feats, images = video_inputs(frames_u8, extractor, image_hw=image_hw)
    feats = np.asarray(feats, np.float32).reshape(len(feats), 1024, 7, 7)
    return predict_long_clips(model, [feats], frames=[images])[0]
