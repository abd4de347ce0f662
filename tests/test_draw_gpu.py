"""GPU: the track overlay - visualization.draw_tracks on st_draw_tracks (csrc/draw_tracks.hip) equals tests/draw_ref.py
byte for byte, inside guard bands; and the visualisation config end to end on the tiny dataset."""
import os
import sys

import numpy as np
import pytest
import torch

import draw_ref
import guard_memory as gm
from stream_pool import keep_pool_position  # noqa: F401  (autouse: the streams this module takes shift no later test's)
from stereotracking_amd import jpeg, jpeg_write as jw, visualization as vis

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RED, GREEN, BLUE, GREY, SAND = (10, 20, 250), (30, 200, 40), (240, 60, 5), (127, 127, 127), (34, 189, 188)


def frame(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (3, h, w)).astype(np.uint8)


def scene(h, w):
    """five boxes: crossing every edge of the image (zoom 2 by its area, most of it off the image; its outline shows in
    row 0 and column 0, its tag is clipped by the right border), nested in it, overlapping an earlier one, a zoom-1 tag
    clipped by the right border, entirely off the image"""
    return [((-1.4, -0.8, w + 200.0, h + 150.0), RED, '12 | 0.91'),
            ((4.0, 3.0, w - 6.5, h - 4.5), GREEN, '7'),
            ((8.5, 7.5, 20.49, 19.0), BLUE, '3 | 0.50'),
            ((w - 9.0, 5.0, w - 2.0, 16.0), GREY, '108-.|'),
            ((-40.0, -30.0, -20.0, -10.0), SAND, '5')]


def run(frames_np, per_frame, cuda, **kw):
    """draw_tracks on frames inside guard bands -> the painted frames (numpy); asserts the bands"""
    x = gm.arena(torch.from_numpy(frames_np), device=cuda)
    boxes, counts = vis.pack_boxes(per_frame)
    vis.draw_tracks(x, boxes, counts, **kw)
    torch.cuda.synchronize()
    assert gm.bands_intact(x)
    return x.cpu().numpy()


@pytest.mark.parametrize('hw', [(24, 40), (33, 31)])
@pytest.mark.parametrize('k', [0, 1, 5])
def test_draw_equals_reference(hw, k, cuda):
    h, w = hw
    src = frame(h, w, 3)[None]
    boxes = scene(h, w)[:k]
    assert k < 1 or draw_ref.ref_zoom(boxes[0][0]) == 2
    assert k < 5 or {draw_ref.ref_zoom(b[0]) for b in boxes} == {1, 2}
    got = run(src, [boxes], cuda)
    assert np.array_equal(got[0], draw_ref.draw_ref(src[0], boxes))
    if k:
        assert not np.array_equal(got[0], src[0])
    else:
        assert np.array_equal(got[0], src[0])


def test_zoom_two_tag_inside_the_image(cuda):
    """a frame wide enough to hold a whole zoom-2 tag, and a zoom-1 tag painted over it"""
    src = frame(40, 200, 5)[None]
    boxes = [((2.0, 2.0, 190.0, 180.0), RED, '42 | 1.00'), ((100.2, 1.0, 140.0, 30.0), BLUE, '9')]
    assert [draw_ref.ref_zoom(b[0]) for b in boxes] == [2, 1]
    got = run(src, [boxes], cuda)
    assert np.array_equal(got[0], draw_ref.draw_ref(src[0], boxes))
    assert (got[0][:, 5 + 2:5 + 16, 5 + 2:5 + 100] == 0).any()           # ink


def test_order_matters_and_is_the_lists(cuda):
    src = frame(24, 40, 6)[None]
    a, b = ((3.0, 3.0, 25.0, 18.0), RED, '1'), ((10.0, 6.0, 35.0, 21.0), GREEN, '2')
    ab, ba = run(src, [[a, b]], cuda)[0], run(src, [[b, a]], cuda)[0]
    assert np.array_equal(ab, draw_ref.draw_ref(src[0], [a, b]))
    assert np.array_equal(ba, draw_ref.draw_ref(src[0], [b, a]))
    assert not np.array_equal(ab, ba)


def test_three_frames_with_different_counts_line_width_alpha(cuda):
    h, w = 33, 31
    src = np.stack([frame(h, w, 10 + i) for i in range(3)])
    per_frame = [scene(h, w), [], scene(h, w)[2:4]]
    for kw in (dict(), dict(line_width=1, alpha=1.0), dict(line_width=4, alpha=0.35)):
        got = run(src, per_frame, cuda, **kw)
        for i in range(3):
            assert np.array_equal(got[i], draw_ref.draw_ref(src[i], per_frame[i], **kw)), (i, kw)
    assert np.array_equal(got[1], src[1])


def test_strided_frames_and_degenerate_boxes(cuda):
    """frames as a view into a wider buffer; non-finite and inverted boxes paint nothing, a 1-pixel box paints 3x3"""
    h, w = 24, 40
    wide = gm.arena(torch.full((2, 4, h + 5, w + 7), 0xEE, dtype=torch.uint8), device=cuda)
    view = wide[:, 1:4, 3:3 + h, 4:4 + w]
    src = np.stack([frame(h, w, 20), frame(h, w, 21)])
    view.copy_(torch.from_numpy(src).to(cuda))
    boxes = [((float('nan'), 1.0, 5.0, 5.0), RED, '1'), ((9.0, 9.0, 3.0, 12.0), RED, '1'),
             ((float('inf'), 1.0, 5.0, 5.0), RED, '1'), ((12.0, 12.0, 12.0, 12.0), BLUE, '')]
    packed, counts = vis.pack_boxes([boxes, boxes[:2]])
    vis.draw_tracks(view, packed, counts)
    torch.cuda.synchronize()
    assert gm.bands_intact(wide)
    got = view.cpu().numpy()
    assert np.array_equal(got[0], draw_ref.draw_ref(src[0], boxes))
    assert np.array_equal(got[1], src[1])
    assert int((got[0] != src[0]).any(0).sum()) <= 9
    outside = torch.ones_like(wide, dtype=torch.bool)
    outside[:, 1:4, 3:3 + h, 4:4 + w] = False
    assert bool((wide[outside] == 0xEE).all())


def test_vis_config_end_to_end_on_the_tiny_dataset(tmp_path, cuda):
    """the visualisation config's hook on the tiny dataset's frames: one decodable file per frame, and frame 0 decodes
    to what the host encoder makes of draw_ref's painting of it"""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import vis_demo
    finally:
        sys.path.pop(0)
    cfg = os.path.join(ROOT, 'configs', 'stereo_tracking', 'ocsort', 'yolox_s_mmyolo_mot_airdrone_disp_vis.py')
    record = vis_demo.run(cfg, str(tmp_path / 'data'), str(tmp_path / 'out'), frames=3, device=cuda, score_thr=0.0)
    assert len(record) == 3 and sum(len(r['boxes']) for r in record) > 0
    assert sorted(os.listdir(tmp_path / 'out')) == ['000000.jpg', '000001.jpg', '000002.jpg']
    for r in record:
        assert os.path.isfile(r['file']) and r['file'].endswith('.jpg')
        assert jpeg.read_jpeg(r['file']).shape == (r['height'], r['width'], 3)
    r = record[0]
    painted = draw_ref.draw_ref(r['frame_bgr'], [(b, rgb[::-1], label) for b, rgb, label in r['boxes']])
    want = jw.encode_jpeg_host(np.ascontiguousarray(painted.transpose(1, 2, 0)), r['quality'], r['subsampling'], order='bgr')
    assert np.array_equal(jpeg.read_jpeg(r['file']), jpeg.read_jpeg(want))
