"""GPU: the collect stage on the device (vp_collect_stream / vp_collect, VitPoseHip.collect / collect_host) against the host model of the same header
(vp_dbg_collect_host, pinned on the CPU against its numpy restatement and literal anchors: tests/test_collect_host.py).  Every comparison is over every byte of
the table: words are copied, never computed, so equal means equal."""
from __future__ import annotations

import numpy as np
import pytest

from easy_vitpose_amd import VitPoseHip
from easy_vitpose_amd import _capi as capi
from easy_vitpose_amd import devcollect as dv
from easy_vitpose_amd.configs import model_shape
from easy_vitpose_amd.devcollect import collect_tap, parse_records
from easy_vitpose_amd.synth import synthetic_state_dict
import collect_cases as cc

pytestmark = pytest.mark.gpu
CASES = cc.host_cases()


@pytest.fixture(scope='module')
def eng():
    shp = model_shape('s', 'coco')
    e = VitPoseHip(shp, synthetic_state_dict(shp, 0, peaked=True), dtype='fp16', max_batch=8)
    yield e
    e.close()


def to_device(cs):
    """the case on torch tensors: the score, when strided, as the column view of its uploaded table"""
    import torch
    kw = {}
    for k, v in cs.items():
        if not isinstance(v, np.ndarray):
            kw[k] = v
        elif k == 'score' and v.base is not None and v.strides[0] != 4:
            kw[k] = torch.from_numpy(v.base).cuda()[:, 4]
        else:
            kw[k] = torch.from_numpy(np.ascontiguousarray(v)).cuda()
    return kw


@pytest.mark.parametrize('name', sorted(CASES))
def test_device_equals_the_host_model_on_the_cpu_cases(eng, name):
    cs = CASES[name]
    nbytes = len(collect_tap(**cs))
    got, want = dv.aligned_bytes(nbytes + 64, fill=0xA5), dv.aligned_bytes(nbytes + 64, fill=0xA5)
    eng.collect_host(**cs, out=got)
    collect_tap(**cs, out=want)
    assert np.array_equal(got, want), f'{name}: {int((got != want).sum())} bytes differ'


def test_every_combination_of_null_inputs(eng):
    for name, cs in cc.null_combos().items():
        assert np.array_equal(eng.collect_host(**cs), collect_tap(**cs)), name


def test_stream_entry_with_the_score_as_column_4_of_the_rows(eng):
    import torch
    cs = CASES['strided_score']
    assert cs['score'].strides[0] == 24
    kw = to_device(cs)
    assert kw['score'].stride(0) == 6
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        table = eng.collect(**kw)
    side.synchronize()
    want = collect_tap(**cs)
    assert table.dtype == torch.uint8 and table.is_cuda and np.array_equal(table.cpu().numpy(), want)
    rec = parse_records(table.cpu().numpy(), cs['n_frames'], 17)
    assert rec.total > 3 and np.array_equal(rec.score, cs['score'][rec.row])


@pytest.mark.parametrize('name,max_records', [('plain', 4), ('plain', None), ('plain', 0), ('k133', 2), ('n0', 0)])
def test_the_tail_behind_the_last_record_is_untouched(eng, name, max_records):
    import torch
    cs = dict(CASES[name], max_records=max_records)
    want = dv.aligned_bytes(len(collect_tap(**cs)) + 4096, fill=0x5A)
    collect_tap(**cs, out=want)
    assert (want[-4096:] == 0x5A).all()
    out = torch.full((len(want),), 0x5A, dtype=torch.uint8, device='cuda')
    kw = to_device(cs)
    eng.collect(**kw, out=out)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize('name', ['chunk_600', 'chunk_1025', 'cap_8192_on_64'])
def test_three_runs_are_bit_identical_on_many_rows(eng, name):
    import torch
    cs = CASES[name]
    kw = to_device(cs)
    want = collect_tap(**cs)
    assert parse_records(want, cs['n_frames'], cs['kpts'].shape[1]).total > len(cs['kpts']) // 8
    runs = []
    for _ in range(3):
        out = torch.full((len(want),), 0x5A, dtype=torch.uint8, device='cuda')
        eng.collect(**kw, out=out)
        runs.append(out)
    torch.cuda.synchronize()
    m = parse_records(want, cs['n_frames'], cs['kpts'].shape[1])
    written = 4 * (dv.header_words(cs['n_frames']) + len(m.ids) * dv.record_words(cs['kpts'].shape[1]))
    for r in runs:
        got = r.cpu().numpy()
        assert np.array_equal(got[:written], want[:written]) and (got[written:] == 0x5A).all()


def test_capture_and_replay_give_the_same_bytes(eng):
    """the stage takes no host input that changes between replays: new rows in the same tensors, the same graph"""
    import torch
    a, b = cc.rows(31, 77, 17, 3), cc.rows(32, 77, 17, 3)
    kw = to_device(a)
    nbytes = dv.collect_bytes(3, 17, 77)
    out = torch.zeros((nbytes,), dtype=torch.uint8, device='cuda')
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        eng.collect(**kw, out=out)   # warm-up outside the capture
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        eng.collect(**kw, out=out)
    for cs in (a, b, a):
        for k, v in cs.items():
            if isinstance(v, np.ndarray):
                kw[k].copy_(torch.from_numpy(np.ascontiguousarray(v)).cuda())
        out.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), collect_tap(**cs))


def test_refusals_come_before_anything_is_enqueued(eng):
    import torch
    kp = torch.zeros((2, 17, 3), device='cuda')
    out = torch.full((1024,), 7, dtype=torch.uint8, device='cuda')

    def call(kpts=kp.data_ptr(), n=2, k=17, stride=1, n_frames=1, max_records=2, out_=out.data_ptr()):
        rc = eng.lib.vp_collect_stream(eng._h, kpts, n, k, None, None, None, None, None, stride, None, n_frames, max_records, out_, None)
        return rc, capi.last_error(eng._h)
    for kw, msg in ((dict(n=8193), 'n = 8193 rows outside 0..8192'), (dict(n_frames=65), 'n_frames = 65 outside 1..64'), (dict(k=134), 'k = 134 joints outside 1..133'),
                    (dict(max_records=-1), 'negative max_records'), (dict(kpts=None), 'null keypoints with n > 0'), (dict(out_=None), 'null output'),
                    (dict(stride=0), 'a score stride < 1'), (dict(out_=out.data_ptr() + 8), 'the output is not 16-byte aligned')):
        rc, why = call(**kw)
        assert rc == capi.VP_ERR_INVALID and why == 'collect: ' + msg, (kw, why)
    torch.cuda.synchronize()
    assert (out == 7).all()
    with pytest.raises(TypeError, match='kpts'):
        eng.collect(np.zeros((2, 17, 3), np.float32))
    with pytest.raises(ValueError, match='ids'):
        eng.collect(kp, ids=torch.zeros(3, dtype=torch.int32, device='cuda'))
    with pytest.raises(ValueError, match='out'):
        eng.collect(kp, out=out[8:])
    assert call()[0] == capi.VP_OK
    torch.cuda.synchronize()
    assert out[:16].view(torch.int32).tolist() == [2, 2, 0, 0]
