"""GPU: the gaze-map export (csrc/rgp_mapexport.hip through models/extract_map.py) against the numpy oracle of
tests/export_ref.py, which tests/test_export_cpu.py pins to Pillow at these shapes (the GPU box may have no Pillow).

The claim is equality: the bytes of both 8-bit outputs, and the float64 quotients bit for bit (through .view(np.int64);
NaN cells, which a zero sum makes, are compared by position).  The cases are tests/export_cases.py's."""
import ctypes

import numpy as np
import pytest
import torch

import export_cases as cases
import export_ref as ref
from recurrent_gaze_prediction_amd import _lib
from recurrent_gaze_prediction_amd import frames as fr
from recurrent_gaze_prediction_amd import synthetic as syn
from recurrent_gaze_prediction_amd.models import extract_map as em

pytestmark = pytest.mark.gpu


def report(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    if want.dtype == np.float64:
        bad = int((np.isnan(got) != np.isnan(want)).sum() + (got.view(np.int64) != want.view(np.int64))[~np.isnan(want) & ~np.isnan(got)].sum())
    else:
        bad = int((got != want).sum())
    print('%s: %d of %d cells differ' % (name, bad, want.size))


def check_all_three(d_maps, out, filt, want, tag):
    pooled, small, u8 = want
    got = em._export(d_maps, out, filt, ('pooled', 'pooled_u8', 'bytes'), None)
    g_pooled, g_small, g_u8 = got['pooled'].cpu().numpy(), got['pooled_u8'].cpu().numpy(), got['bytes'].cpu().numpy()
    assert g_pooled.dtype == np.float64 and g_pooled.shape == pooled.shape
    assert g_small.dtype == np.uint8 and g_small.shape == small.shape and g_u8.dtype == np.uint8 and g_u8.shape == u8.shape
    report(tag + ' bytes', g_u8, u8)
    report(tag + ' pooled_u8', g_small, small)
    report(tag + ' pooled', g_pooled, pooled)
    assert np.array_equal(g_u8, u8)
    assert np.array_equal(g_small, small)
    assert ref.same_float64(g_pooled, pooled)
    return got


@pytest.mark.parametrize('hw, out, n', cases.CASES, ids=cases.IDS)
def test_all_three_outputs_equal_the_oracle(gpu, hw, out, n):
    maps = cases.maps(hw, n)
    d_maps = torch.from_numpy(np.array(maps)).to(gpu)
    got = check_all_three(d_maps, out, 'bilinear', cases.oracle(hw, out, n), '%s->%s n=%d' % (hw, out, n))
    pooled = cases.oracle(hw, out, n)[0]
    for i in range(n):                                    # NaN only where the case was made for it (or the oracle says so)
        if cases.kind_of(i) in cases.RANDOM_KINDS:
            assert np.isfinite(pooled[i]).all()
        if cases.kind_of(i) in cases.NAN_KINDS:
            assert np.isnan(pooled[i]).all()
    # one output at a time: the same bits
    assert torch.equal(em.bytescale_maps(d_maps), got['bytes'])
    assert torch.equal(em._export(d_maps, out, 'bilinear', ('pooled_u8',), None)['pooled_u8'], got['pooled_u8'])
    alone = em.avg_pool(d_maps, out)
    assert alone.is_cuda and alone.dtype == torch.float64 and ref.same_float64(alone.cpu().numpy(), got['pooled'].cpu().numpy())


@pytest.mark.parametrize('filt', ['lanczos', 'bicubic'])
def test_the_other_filters(gpu, filt):
    for hw, out, n in (((49, 49), (7, 7), 5), ((49, 48), (7, 3), 67)):
        d_maps = torch.from_numpy(np.array(cases.maps(hw, n))).to(gpu)
        check_all_three(d_maps, out, filt, cases.oracle(hw, out, n, filt), '%s %s->%s n=%d' % (filt, hw, out, n))


def test_device_tensor_and_numpy_agree(gpu):
    hw, out, n = (49, 49), (7, 7), 67
    maps = np.array(cases.maps(hw, n))
    pooled, small, u8 = cases.oracle(hw, out, n)
    from_host, bytes_host = em.avg_pool(maps, return_bytes=True, device=gpu)
    from_dev, bytes_dev = em.avg_pool(torch.from_numpy(maps).to(gpu), return_bytes=True)
    assert isinstance(from_host, np.ndarray) and from_host.dtype == np.float64 and from_host.shape == (n, 7, 7)
    assert isinstance(bytes_host, np.ndarray) and bytes_host.dtype == np.uint8
    assert from_dev.is_cuda and bytes_dev.is_cuda
    assert ref.same_float64(from_host, from_dev.cpu().numpy()) and ref.same_float64(from_host, pooled)
    assert np.array_equal(bytes_host, bytes_dev.cpu().numpy()) and np.array_equal(bytes_host, u8)
    assert ref.same_float64(em.avg_pool(torch.from_numpy(maps), device=gpu), pooled)            # a host tensor: numpy back
    assert np.array_equal(em.bytescale_maps(maps, device=gpu), u8)
    # a contiguous slice of maps starts 4-byte aligned only
    d = torch.from_numpy(maps).to(gpu)
    assert ref.same_float64(em.avg_pool(d[3:]).cpu().numpy(), pooled[3:])
    with pytest.raises(ValueError, match='contiguous'):
        em.avg_pool(d[:, :, ::2])


def test_a_nan_map_and_inf_maps_are_refused_and_their_neighbours_are_exact(gpu):
    hw, out, n = (49, 49), (7, 7), 67
    maps = np.array(cases.maps(hw, n))
    pooled, small, u8 = (np.array(a) for a in cases.oracle(hw, out, n))
    maps[2, 17, 30] = np.nan
    maps[4, 0, 0] = np.inf
    maps[65, 48, 48] = -np.inf
    refused = [2, 4, 65]
    rest = [i for i in range(n) if i not in refused]
    with pytest.raises(_lib.RgpError) as info:
        em._export(torch.from_numpy(maps).to(gpu), out, 'bilinear', ('pooled', 'pooled_u8', 'bytes'), None)
    assert info.value.code == -1 and '3 map(s) refused' in str(info.value)
    got = {k: v.cpu().numpy() for k, v in info.value.outputs.items()}
    assert np.isnan(got['pooled'][refused]).all() and not got['pooled_u8'][refused].any() and not got['bytes'][refused].any()
    assert ref.same_float64(got['pooled'][rest], pooled[rest])
    assert np.array_equal(got['pooled_u8'][rest], small[rest]) and np.array_equal(got['bytes'][rest], u8[rest])
    with pytest.raises(_lib.RgpError, match=r'1 map\(s\) refused'):
        em.bytescale_maps(maps[:3], device=gpu)
    # the next clean call returns normally
    assert ref.same_float64(em.avg_pool(np.array(cases.maps(hw, 5)), device=gpu), cases.oracle(hw, out, 5)[0])


def test_the_status_word_and_a_bad_bounds_table(gpu):
    """Straight to the C entry: the status word counts; a bounds table with an entry past the map refuses every map before
    anything is read through it."""
    hw, out, n = (49, 48), (7, 3), 5
    maps = np.array(cases.maps(hw, n))
    pooled, small, u8 = cases.oracle(hw, out, n)
    lib = _lib.load()
    kh, bh, ksh = fr.resample_coeffs(48, 3, 'bilinear')
    kv, bv, ksv = fr.resample_coeffs(49, 7, 'bilinear')
    stream = torch.cuda.current_stream(gpu).cuda_stream

    def run(bh_host, bv_host):
        t = [torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in (kh, bh_host, kv, bv_host, maps)]
        o_small = torch.full((n, 7, 3), 7, dtype=torch.uint8, device=gpu)
        o_pooled = torch.zeros((n, 7, 3), dtype=torch.float64, device=gpu)
        ws = torch.empty(lib.rgp_mapexport_workspace_bytes(), dtype=torch.uint8, device=gpu)
        args = _lib.MapExportArgs(maps=t[4].data_ptr(), n=n, h=49, w=48, out_h=7, out_w=3, kh=t[0].data_ptr(), bh=t[1].data_ptr(),
                                  ksize_h=ksh, kv=t[2].data_ptr(), bv=t[3].data_ptr(), ksize_v=ksv, pooled=o_pooled.data_ptr(),
                                  pooled_u8=o_small.data_ptr(), bytes=None, workspace=ws.data_ptr(), workspace_bytes=ws.numel())
        assert lib.rgp_mapexport(ctypes.byref(args), stream) == 0
        count = ctypes.c_int(-7)
        rc = lib.rgp_mapexport_status(ws.data_ptr(), ctypes.byref(count), stream)
        return rc, count.value, o_small.cpu().numpy(), o_pooled.cpu().numpy()

    rc, count, o_small, o_pooled = run(bh, bv)
    assert rc == 0 and count == 0 and np.array_equal(o_small, small) and ref.same_float64(o_pooled, pooled)
    for table, row, col, value in (('v', 6, 1, int(bv[6, 1]) + 1), ('v', 3, 0, -1), ('h', 2, 1, int(bh[2, 1]) + 1), ('h', 0, 0, -1),
                                   ('h', 1, 1, ksh + 1), ('v', 0, 1, -2)):
        bad_h, bad_v = bh.copy(), bv.copy()
        (bad_h if table == 'h' else bad_v)[row, col] = value
        rc, count, o_small, o_pooled = run(bad_h, bad_v)
        assert rc == -1 and count == n and not o_small.any() and np.isnan(o_pooled).all(), (table, row, col, value)
        assert b'5 map(s) refused' in lib.rgp_last_error()


def test_no_maps(gpu):
    empty = torch.zeros((0, 49, 49), dtype=torch.float32, device=gpu)
    pooled, u8 = em.avg_pool(empty, return_bytes=True)
    assert tuple(pooled.shape) == (0, 7, 7) and pooled.dtype == torch.float64 and tuple(u8.shape) == (0, 49, 49) and pooled.is_cuda
    assert em.bytescale_maps(np.zeros((0, 14, 14), np.float32), device=gpu).shape == (0, 14, 14)
    lib = _lib.load()
    assert lib.rgp_mapexport(ctypes.byref(_lib.MapExportArgs(n=0)), torch.cuda.current_stream(gpu).cuda_stream) == 0


# ---------------------------------------------------------------------------------------------------- through a model
def make_model(gpu, tmp_path, B=2, T=4):
    """The smallest plan the evaluation tests build (tests/test_evaluate_gpu.py)."""
    from recurrent_gaze_prediction_amd.models.base import Session
    from recurrent_gaze_prediction_amd.models.gaze_grcn import GazePredictionGRCN, GRUModelConfig
    cfg = GRUModelConfig()
    cfg.batch_size, cfg.n_lstm_steps, cfg.compute_dtype, cfg.train_dir, cfg.trainable = B, T, 'bf16', str(tmp_path), False
    ds = type('DS', (), {})()
    ds.train = ds.valid = syn.SyntheticDataSet(8, T, seed=21)
    m = GazePredictionGRCN(Session(gpu), ds, cfg)
    m.load_state_dict(syn.grcn_params(22, T, gru_std=0.05, random_bn=True))
    return m


def test_predict_long_clip_imresize_and_export_clips(gpu, tmp_path):
    from recurrent_gaze_prediction_amd.models.evaluate_gaze import predict_long_clip
    model = make_model(gpu, tmp_path / 'model')
    n = 11                                                     # 2 full chunks of T = 4 and a zero-padded tail of 3
    feats = syn.c3d_features(31, 1, n)[0]
    for carry in (False, True):
        maps = predict_long_clip(model, feats, carry_state=carry)
        assert maps.shape == (n, 49, 49) and maps.dtype == np.float32
        want = ref.avg_pool(np.ascontiguousarray(maps))[0]
        got = predict_long_clip(model, feats, pool_to_7x7='imresize', carry_state=carry)
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (n, 7, 7)
        assert np.isfinite(want).all() and ref.same_float64(got, want), carry
        mean = predict_long_clip(model, feats, pool_to_7x7=True, carry_state=carry)            # unchanged: the block mean
        assert mean.shape == (n, 7, 7) and np.array_equal(mean, maps.reshape(n, 7, 7, 7, 7).mean(axis=(2, 4)))
        assert not np.array_equal(mean, got)
    with pytest.raises(ValueError, match='pool_to_7x7'):
        predict_long_clip(model, feats, pool_to_7x7='mean')
    # the export: three clips, B = 2 per predict, one longer than T
    chunked = predict_long_clip(model, feats)
    clips = [('a', feats[:4]), ('b', feats[4:8]), ('c', feats[:3]), ('d', feats[2:9])]
    out_dir = str(tmp_path / 'gazemaps')
    assert em.export_clips(model, clips, out_dir) == ['a', 'b', 'c', 'd']
    m49 = np.load(tmp_path / 'gazemaps' / 'a' / 'a.gazemap.49.npy')
    m77 = np.load(tmp_path / 'gazemaps' / 'a' / 'a.gazemap.npy')
    assert m49.dtype == np.float32 and np.array_equal(m49, chunked[:4])
    assert m77.dtype == np.float64 and ref.same_float64(m77, ref.avg_pool(m49)[0])
    for name, length in (('b', 4), ('c', 3), ('d', 4)):
        m49 = np.load(tmp_path / 'gazemaps' / name / ('%s.gazemap.49.npy' % name))
        m77 = np.load(tmp_path / 'gazemaps' / name / ('%s.gazemap.npy' % name))
        assert m49.shape == (length, 49, 49) and m77.shape == (length, 7, 7)
        assert ref.same_float64(m77, ref.avg_pool(m49)[0])


def test_run_evaluation_dumps_scipys_bytes_with_the_device_scorer(gpu, tmp_path, monkeypatch):
    pytest.importorskip('PIL.Image')
    from recurrent_gaze_prediction_amd.models import evaluate_gaze as eg
    model = make_model(gpu, tmp_path / 'model')
    ds = type('DS', (), {})()
    ds.train = ds.valid = syn.SyntheticDataSet(8, 4, seed=21)
    seen = []
    write = eg._write_frame

    def spy(i, n_images, image, pred, gt, scores, out_dir, dump_images, dump_scale='minmax', pred_bytes=None):
        seen.append((np.array(pred), dump_scale, None if pred_bytes is None else np.array(pred_bytes)))
        return write(i, n_images, image, pred, gt, scores, out_dir, dump_images, dump_scale, pred_bytes)
    monkeypatch.setattr(eg, '_write_frame', spy)
    out = str(tmp_path / 'eval')
    eg.run_evaluation(model, ds, out, num_frames=12, seed=3, dump_images=True, scorer='device', dump_scale='bytescale')
    assert len(seen) == 16
    for pred, scale, given in seen:
        assert scale == 'bytescale' and given is not None and np.array_equal(given, ref.bytescale(pred))
    assert (tmp_path / 'eval' / '00000.gaze_pred.jpg').exists()
    with pytest.raises(ValueError, match='dump_scale'):
        eg.run_evaluation(model, ds, out, num_frames=4, dump_scale='round')
