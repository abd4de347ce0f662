"""CPU: the host half of stereotracking_amd/_packed.py (the layout of a packed buffer and its binding to an args
struct) and mot_eval's decoder of the device status words.  No launch: buffers and status words are built by hand."""
import ctypes as C

import numpy as np
import pytest

from stereotracking_amd import _lib, mot_eval
from stereotracking_amd._packed import _Layout

ARRAYS = dict(rows=np.arange(42, dtype=np.float64).reshape(7, 6) / 3, none=np.zeros((0, 6)), off=np.array([0, 3, 7], np.int32),
              big=np.array([2 ** 40 + 1, -5], np.int64), one=np.arange(256, dtype=np.uint8), keep=np.array([[1, 0, 1]], np.uint8))


def _layout():
    return _Layout((k, v.shape, v.dtype) for k, v in ARRAYS.items())


def test_offsets_are_multiples_of_256_with_a_256_byte_gap():
    lay = _layout()
    end = 0
    for name, (off, shape, dtype) in lay.items.items():
        assert off % 256 == 0 and off == end, name
        assert shape == ARRAYS[name].shape and dtype == ARRAYS[name].dtype
        end = off + (ARRAYS[name].nbytes + 255) // 256 * 256 + 256       # rounded up, then one 256-byte gap
    assert lay.size == end
    assert [lay.items[k][0] for k in ARRAYS] == [0, 768, 1024, 1536, 2048, 2560] and lay.size == 3072


def test_fill_and_view_round_trip_over_mixed_dtypes():
    lay = _layout()
    buf = lay.fill(ARRAYS)
    assert buf.dtype == np.uint8 and buf.shape == (lay.size,)
    used = np.zeros(lay.size, bool)
    for name, a in ARRAYS.items():
        v = lay.view(buf, name)
        assert v.dtype == a.dtype and v.shape == a.shape and v.tobytes() == a.tobytes(), name
        used[lay.items[name][0]:lay.items[name][0] + a.nbytes] = True
    assert lay.view(buf, 'none').size == 0 and int(lay.view(buf, 'big')[0]) == 2 ** 40 + 1
    assert not buf[~used].any()                   # what no array covers stays zero
    lay.view(buf, 'off')[1] = 9                   # a view, not a copy
    assert lay.view(buf, 'off').tolist() == [0, 9, 7]


class _Args(C.Structure):
    _fields_ = [('n', C.c_int)] + [(k, C.c_void_p) for k in ('rows', 'none', 'off', 'big', 'one', 'keep', 'ws')]


def test_bind_sets_base_plus_offset_for_the_selected_names_only():
    lay, base = _layout(), 0x7f0000001000
    args = _Args()
    lay.bind(args, base, ('off', 'big'))
    assert args.off == base + 1024 and args.big == base + 1536
    assert all(getattr(args, k) is None for k in ('rows', 'none', 'one', 'keep', 'ws')) and args.n == 0
    lay.bind(args, base, ())
    assert args.rows is None
    lay.bind(args, base)                          # default: every array of the layout
    assert [getattr(args, k) for k in ARRAYS] == [base + lay.items[k][0] for k in ARRAYS] and args.ws is None


def test_every_entry_refuses_to_run_without_a_device(monkeypatch):
    import torch
    from stereotracking_amd.aflink import AppearanceFreeLink
    from stereotracking_amd.tracklets import InterpolateTracklets
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    rows = np.array([[f, 1, 0, 0, 9, 9, 1] for f in range(1, 5)], np.float64)
    packed = mot_eval.pack_sequences([rows[:, :6]], [rows[:, :6]])
    for what, source, call in (
            ('the MOT evaluation', 'csrc/mot_eval.hip', lambda: mot_eval.evaluate_packed(packed)),
            ('the KITTI preprocessing', 'csrc/mot_eval.hip', lambda: mot_eval.kitti_keep_masks([], [])),
            ('the MOTChallenge protocol', 'csrc/mot_eval.hip', lambda: mot_eval.motchallenge_keep_masks([rows], [rows])),
            ('the MOTChallenge protocol', 'csrc/mot_eval.hip', lambda: mot_eval.evaluate_motchallenge([rows], [rows])),
            ('InterpolateTracklets', 'csrc/tracklet_post.hip', lambda: InterpolateTracklets(backend='device').forward(rows)),
            ('AppearanceFreeLink', 'csrc/aflink.hip', lambda: AppearanceFreeLink(None, backend='device').forward(rows))):
        with pytest.raises(RuntimeError) as e:
            call()
        assert str(e.value) == (f'the device backend of {what} runs on the HIP path only ({source}) and no CUDA (ROCm) device '
                                f"is available; use backend='host'")


# ---- the status words: word 0 = the bits, word 1 + k = (number of frames - the first frame with bit 1 << k) -------------
VIDEOS = ['a', 'b', 'c']
FRAME_SEQ = np.array([0, 0, 1, 2, 2, 2], np.int32)
FRAME_NO = np.array([3, 9, 1, 4, 5, 8], np.int64)
PER_FRAME = ' (at most {n} ground-truth and {n} prediction rows per frame)'          # the note of bit 8, as the entries pass it
TABLES = [('MOT evaluation', mot_eval.STATUS_KINDS, PER_FRAME),
          ('KITTI preprocessing', mot_eval.KITTI_STATUS_KINDS,
           ' (at most {n} ground-truth rows of a class and its distractors and {n} prediction rows of the class per frame)'),
          ('MOTChallenge preprocessing', mot_eval.CHALLENGE_STATUS_KINDS, PER_FRAME)]


def _status(bits, frame_of_bit):
    st = np.zeros(8, np.int32)
    st[0] = bits
    for bit, f in frame_of_bit.items():
        st[1 + bit.bit_length() - 1] = len(FRAME_NO) - f
    return st


def _raise(prefix, kinds, note, status):
    mot_eval._raise_status(prefix, kinds, status, VIDEOS, FRAME_SEQ, FRAME_NO, note)


def test_the_tables_name_the_bits_of_the_header():
    assert [b for b, _ in mot_eval.STATUS_KINDS] == [1, 2, 4, 8, 16]
    assert [b for b, _ in mot_eval.KITTI_STATUS_KINDS] == [b for b, _ in mot_eval.CHALLENGE_STATUS_KINDS] == [1, 8, 32]
    assert mot_eval.max_frame_objects() == 256


@pytest.mark.parametrize('prefix,kinds,note', TABLES, ids=[t[0] for t in TABLES])
def test_every_bit_names_its_video_and_frame(prefix, kinds, note):
    for k, (bit, what) in enumerate(kinds):
        f = (2 * k + 1) % len(FRAME_NO)           # another frame for every bit
        error = ValueError if bit in (1, 2, 8) else _lib.StError
        with pytest.raises(error) as e:
            _raise(prefix, kinds, note, _status(bit, {bit: f}))
        assert type(e.value) is error
        assert str(e.value) == (f'{prefix}: {what}: video {VIDEOS[FRAME_SEQ[f]]!r}, frame {FRAME_NO[f]}' +
                                (note.format(n=256) if bit == 8 else ''))


@pytest.mark.parametrize('prefix,kinds,note', TABLES, ids=[t[0] for t in TABLES])
def test_the_first_bit_of_the_table_wins_and_unknown_bits_are_errors(prefix, kinds, note):
    (b0, w0), (b1, _) = kinds[0], kinds[-1]
    with pytest.raises(ValueError, match=f"^{prefix}: {w0}: video 'c', frame 5$"):
        _raise(prefix, kinds, note, _status(b0 | b1, {b0: 4, b1: 0}))
    with pytest.raises(_lib.StError, match=f'^{prefix} failed on the device: status 64$'):
        _raise(prefix, kinds, note, _status(64, {}))
