"""The visualisation surface without a GPU (stereotracking_amd/visualization.py): colour, label and threshold rules, the
side-by-side layout, the hook's interval / names / no-op, the registries and configs - with the two device seams of
TrackLocalVisualizer (_draw, _encode) replaced by the host routines - and tests/draw_ref.py against hand-written cases."""
import os
import re

import numpy as np
import pytest
import torch

import draw_ref
from stereotracking_amd import jpeg, jpeg_write as jw, visualization as vis
from stereotracking_amd.config import Config
from stereotracking_amd.registry import HOOKS, VISUALIZERS
from stereotracking_amd.structures import InstanceData, TrackDataSample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_DIR = os.path.join(ROOT, 'configs', 'stereo_tracking', 'ocsort')


class HostVisualizer(vis.TrackLocalVisualizer):
    """the device seams on the host: draw_ref for st_draw_tracks, encode_jpeg_host for JpegEncoder"""

    def __init__(self, **kw):
        super().__init__(device='cpu', **kw)
        self.launches, self.encodes = [], []

    def _draw(self, frames, boxes, counts):
        self.launches.append((tuple(frames.shape), boxes.copy(), counts.copy()))
        out = frames.numpy().copy()
        for n in range(len(out)):
            listed = [(b['xyxy'], b['colour'], bytes(b['label'][:b['label_len']]).decode(), int(b['zoom'])) for b in boxes[n, :counts[n]]]
            out[n] = draw_ref.draw_ref(out[n], listed, self.line_width, self.alpha)
        return torch.from_numpy(out)

    def _encode(self, frames):
        self.encodes.append(tuple(frames.shape))
        return [jw.encode_jpeg_host(np.ascontiguousarray(f.numpy().transpose(1, 2, 0)), self.quality, self.subsampling, order='bgr')
                for f in frames]


def sample(ids=(3, 11), scores=(0.9, 0.2), gt=True, path='val/seq00/left/000004.png'):
    s = TrackDataSample(dict(frame_id=4, img_path=path))
    boxes = torch.tensor([[4.0, 5.0, 30.0, 25.0], [20.0, 8.0, 44.0, 28.0]])[:len(ids)]
    s.pred_track_instances = InstanceData(bboxes=boxes, instances_id=torch.tensor(ids), scores=torch.tensor(scores),
                                          labels=torch.zeros(len(ids), dtype=torch.long))
    if gt:
        s.gt_instances = InstanceData(bboxes=boxes[:1] + 1.0, instances_id=torch.tensor(ids[:1]), labels=torch.zeros(1, dtype=torch.long))
    return s


def image(h=32, w=48, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3)).astype(np.uint8)          # RGB, as the reference's


# ---- rules -----------------------------------------------------------------------------------------------------------
def test_colour_per_id_is_the_reference_rule():
    for i in (0, 1, 7, 12345):
        state = np.random.get_state()
        np.random.seed(i)
        want = vis.PALETTE[np.random.choice(range(10))]
        np.random.set_state(state)
        assert vis.random_color(i) == want
    before = np.random.get_state()[1].copy()
    vis.random_color(5)
    assert np.array_equal(np.random.get_state()[1], before)          # the global generator is left alone
    assert len(set(vis.PALETTE)) == 10 and all(len(c) == 3 and all(0 <= v <= 255 for v in c) for c in vis.PALETTE)


def test_labels_and_score_threshold():
    s = sample()
    full = vis.instance_boxes(s.pred_track_instances)
    assert [b[2] for b in full] == ['3 | 0.90', '11 | 0.20']
    assert [b[1] for b in full] == [vis.random_color(3), vis.random_color(11)]
    assert [b[2] for b in vis.instance_boxes(s.gt_instances)] == ['3']
    v = HostVisualizer()
    sides = v._sides(s, True, True, 0.3)
    assert [len(x) for x in sides] == [1, 1] and sides[1][0][2] == '3 | 0.90'       # scores > thr only, GT first
    assert [len(x) for x in v._sides(s, False, True, 0.1)] == [2]
    assert [len(x) for x in v._sides(s, False, True, 0.9)] == [0]                   # strictly greater
    sot = InstanceData(bboxes=torch.zeros(2, 4), scores=torch.tensor([0.5, 0.25]))
    assert [(b[1], b[2]) for b in vis.instance_boxes(sot)] == [(vis.random_color(0), '0.50'), (vis.random_color(1), '0.25')]
    with pytest.raises(NotImplementedError, match='masks'):
        vis.instance_boxes(InstanceData(bboxes=torch.zeros(1, 4), masks=torch.zeros(1, 4, 4)))


def test_zoom_follows_the_adaptive_scale():
    assert [vis.tag_zoom(a) for a in (0, 800, 10000, 15400, 1e9)] == [1, 1, 1, 2, 2]       # int(13 * scale) reaches 11 at 0.846
    for a in (0.0, 799.0, 5000.0, 29999.0, 30000.0, 64000.0):
        scale = float(np.clip(0.5 + (a - 800) / (30000 - 800), 0.5, 1.0))
        assert vis.tag_zoom(a) == max(1, (int(13 * scale) + 3) // 7)
    boxes, counts = vis.pack_boxes([[((0, 0, 300, 200), (1, 2, 3), '42 | 0.50')], []])
    assert boxes.shape == (2, 1) and counts.tolist() == [1, 0]
    b = boxes[0, 0]
    assert b['zoom'] == 2 == draw_ref.ref_zoom((0, 0, 300, 200)) and b['colour'].tolist() == [1, 2, 3]
    assert bytes(b['label'][:b['label_len']]) == b'42 | 0.50'
    assert vis.pack_boxes([[((0, 0, 1, 1), (0, 0, 0), '1234567890123456789')]])[0][0, 0]['label_len'] == vis.LABEL_MAX


def test_side_by_side_width_and_painting():
    v = HostVisualizer(quality=100, subsampling='444')
    img, s = image(), sample()
    both = jpeg.read_jpeg(v.add_datasample('x', img, s))
    assert both.shape == (32, 96, 3)                                   # GT left, prediction right
    pred_only = jpeg.read_jpeg(v.add_datasample('x', img, s, draw_gt=False))
    gt_only = jpeg.read_jpeg(v.add_datasample('x', img, s, draw_pred=False))
    assert pred_only.shape == gt_only.shape == (32, 48, 3)
    assert np.array_equal(both[:, :48], gt_only) and np.array_equal(both[:, 48:], pred_only)
    assert len(v.launches) == 3 and v.launches[0][0] == (2, 3, 32, 48) and v.encodes[0] == (1, 3, 32, 96)
    # the prediction side is draw_ref of the frame with the one box above the threshold, colour in plane (BGR) order
    bgr = np.ascontiguousarray(img[..., ::-1].transpose(2, 0, 1))
    want = draw_ref.draw_ref(bgr, [((4.0, 5.0, 30.0, 25.0), vis.random_color(3)[::-1], '3 | 0.90')])
    assert np.array_equal(pred_only, jpeg.read_jpeg(jw.encode_jpeg_host(np.ascontiguousarray(want.transpose(1, 2, 0)), 100, '444', order='bgr')))
    assert np.array_equal(jpeg.read_jpeg(v.add_datasample('x', img, None)), jpeg.read_jpeg(jw.encode_jpeg_host(img, 100, '444')))


def test_image_forms_and_refusals(tmp_path):
    v = HostVisualizer(save_dir=str(tmp_path / 'save'))
    img, s = image(), sample(gt=False)
    planar = torch.from_numpy(np.ascontiguousarray(img[..., ::-1].transpose(2, 0, 1)))
    a = v.add_datasample('n', img, s, draw_gt=False, out_file=str(tmp_path / 'o' / 'a.jpg'), step=7)
    assert a == v.add_datasample('n', planar, s, draw_gt=False) == v.add_datasample('n', planar[None], s, draw_gt=False)
    assert open(tmp_path / 'o' / 'a.jpg', 'rb').read() == a
    assert open(tmp_path / 'save' / 'vis_data' / 'vis_image' / 'n_7.jpg', 'rb').read() == a
    with pytest.raises(NotImplementedError, match='show=True'):
        v.add_datasample('n', img, s, show=True)
    with pytest.raises(TypeError, match='uint8'):
        v.add_datasample('n', img.astype(np.float32), s, draw_gt=False)
    with pytest.raises(AssertionError):
        v.add_datasample('n', img, s)                                  # draw_gt without gt_instances, as the reference
    with pytest.raises(ValueError, match='subsampling'):
        vis.TrackLocalVisualizer(subsampling='411')


def test_batched_call_is_one_launch_and_one_encode_per_chunk():
    v = HostVisualizer(chunk=4)
    imgs = [image(seed=i) for i in range(5)] + [image(16, 24, 9)]
    samples = [sample(gt=False) for _ in imgs]
    blobs = v.add_datasamples(imgs, samples, draw_gt=False)
    assert [x[0] for x in v.launches] == [(4, 3, 32, 48), (1, 3, 32, 48), (1, 3, 16, 24)] and len(v.encodes) == 3
    assert blobs[1] == HostVisualizer().add_datasample('x', imgs[1], samples[1], draw_gt=False)
    with pytest.raises(ValueError, match='images'):
        v.add_datasamples(imgs, samples[:2])


# ---- the hook --------------------------------------------------------------------------------------------------------
def test_hook_draw_false_is_a_no_op():
    class Boom:
        def __getattr__(self, name):
            raise AssertionError('draw=False touched its arguments')
    hook = vis.TrackVisualizationHook(draw=False, test_out_dir='nowhere')
    assert hook.after_test_iter(Boom(), 0, Boom(), Boom()) is None and hook._visualizer is None
    with pytest.raises(NotImplementedError, match='show=True'):
        vis.TrackVisualizationHook(show=True)


def test_hook_interval_names_and_frames(tmp_path):
    v = HostVisualizer()
    hook = vis.TrackVisualizationHook(draw=True, interval=2, score_thr=0.5, test_out_dir=str(tmp_path / 'out'), wait_time=1.0, visualizer=v)
    frames = [torch.from_numpy(image(seed=i)[..., ::-1].transpose(2, 0, 1).copy())[None] for i in range(2)]
    outs = [sample(gt=False, path='a/b/000004.png'), sample(gt=False, path='a/b/000005.jpg')]
    batch = dict(inputs=dict(img=frames))
    assert hook.after_test_iter(None, 0, batch, outs) is None and not v.launches           # (0 + 1) % 2
    files = hook.after_test_iter(None, 1, batch, outs)
    assert files == [str(tmp_path / 'out' / '000004.jpg'), str(tmp_path / 'out' / '000005.jpg')]
    assert len(v.launches) == 1 and v.launches[0][2].tolist() == [1, 1]                     # 0.9 > 0.5, 0.2 is not
    assert jpeg.read_jpeg(files[0]).shape == (32, 48, 3)
    # fp32 frames holding integers are taken, others refused; a frame count that does not match the outputs too
    as_float = dict(inputs=dict(img=torch.cat(frames).float()[:, None]))
    assert hook.after_test_iter(None, 3, as_float, outs) == files
    with pytest.raises(TypeError, match='integers 0..255'):
        hook.after_test_iter(None, 3, dict(inputs=dict(img=[f.float() + 0.5 for f in frames])), outs)
    with pytest.raises(ValueError, match='2 frames for 1 outputs'):
        hook.after_test_iter(None, 3, batch, outs[:1])

    class Runner:
        work_dir, timestamp = str(tmp_path / 'work'), '20240101_000000'
    hook2 = vis.TrackVisualizationHook(draw=True, interval=1, test_out_dir='vis', visualizer=v)
    for k in range(2):                                                                      # joined once, not per iteration
        assert hook2.after_test_iter(Runner, k, batch, outs)[0] == str(tmp_path / 'work' / '20240101_000000' / 'vis' / '000004.jpg')
    assert vis.TrackVisualizationHook.out_name(TrackDataSample(), 12, 1) == '000012_1.jpg'


def test_hook_falls_back_to_img_path_with_the_projects_readers(tmp_path):
    from stereotracking_amd import datasets
    img = image()
    datasets.write_png(str(tmp_path / 'f.png'), img)
    jpeg.write_jpeg(str(tmp_path / 'g.jpg'), img, quality=95, subsampling='444')
    v = HostVisualizer()
    hook = vis.TrackVisualizationHook(draw=True, interval=1, test_out_dir=str(tmp_path / 'out'), visualizer=v)
    files = hook.after_test_iter(None, 0, dict(inputs=dict()), [sample(gt=False, path=str(tmp_path / 'f.png'))])
    assert files == [str(tmp_path / 'out' / 'f.jpg')]
    assert files[0:1] == hook.after_test_iter(None, 0, None, [sample(gt=False, path=str(tmp_path / 'f.png'))])
    direct = HostVisualizer().add_datasample('x', img, sample(gt=False), draw_gt=False, pred_score_thr=0.3)
    assert open(files[0], 'rb').read() == direct
    assert hook.after_test_iter(None, 1, {}, [sample(gt=False, path=str(tmp_path / 'g.jpg'))]) == [str(tmp_path / 'out' / 'g.jpg')]
    with pytest.raises(ValueError, match='no reader'):
        hook.after_test_iter(None, 2, {}, [sample(gt=False, path='x.bmp')])


# ---- registries and configs ------------------------------------------------------------------------------------------
def test_registered_under_both_names_and_configs_build():
    for reg, cls in ((VISUALIZERS, vis.TrackLocalVisualizer), (HOOKS, vis.TrackVisualizationHook)):
        assert reg.get(cls.__name__) is cls and reg.get('mmtrack.' + cls.__name__) is cls
        assert 'mmtrack.' + cls.__name__ in reg._modules
    for name, draw in (('yolox_s_mmyolo_mot_airdrone_disp.py', False), ('yolox_s_mmyolo_mot_airdrone_disp_vis.py', True)):
        cfg = Config.fromfile(os.path.join(CFG_DIR, name))
        v = VISUALIZERS.build(cfg.visualizer)
        hook = HOOKS.build(cfg.default_hooks.visualization)
        assert isinstance(v, vis.TrackLocalVisualizer) and (v.line_width, v.alpha, v.name) == (3, 0.8, 'visualizer')
        assert isinstance(hook, vis.TrackVisualizationHook) and hook.draw is draw
        assert hook.visualizer is v                                                         # the current instance, as the reference's
    assert cfg.default_hooks.visualization.test_out_dir == 'vis' and hook.interval == 1
    base = Config.fromfile(os.path.join(CFG_DIR, 'yolox_s_mmyolo_mot_airdrone_disp.py'))
    assert cfg.model == base.model                                                          # the model is not touched


# ---- the drawing oracle against hand-written cases -------------------------------------------------------------------
def grey(h, w, v=100):
    return np.full((3, h, w), v, np.uint8)


def painted(out, src):
    return (out != src).any(0)


def test_draw_ref_one_pixel_box():
    src = grey(9, 9)
    out = draw_ref.draw_ref(src, [((4.2, 3.6, 4.4, 4.3), (200, 0, 50), '')], line_width=3, alpha=0.8)
    want = np.zeros((9, 9), bool)
    want[3:6, 3:6] = True                                             # rounds to (4, 4, 4, 4): a 3x3 square
    assert np.array_equal(painted(out, src), want)
    a = round(0.8 * 256)
    assert out[:, 4, 4].tolist() == [(a * c + (256 - a) * 100 + 128) >> 8 for c in (200, 0, 50)]
    assert np.array_equal(painted(draw_ref.draw_ref(src, [((4, 4, 4, 4), (0, 0, 0), '')], line_width=1), src), np.eye(9, dtype=bool) & (np.arange(9) == 4))


def test_draw_ref_box_off_the_image_and_degenerate_boxes():
    src = grey(8, 8)
    for box in ((-30.0, -30.0, -10.0, -10.0), (20.0, 2.0, 40.0, 6.0), (5.0, 5.0, 2.0, 7.0), (float('nan'), 0.0, 4.0, 4.0),
                (0.0, 0.0, float('inf'), 4.0)):
        assert np.array_equal(draw_ref.draw_ref(src, [(box, (255, 255, 255), '8')]), src), box


def test_draw_ref_box_crossing_every_edge():
    src = grey(10, 12)
    out = draw_ref.draw_ref(src, [((0.0, 0.0, 11.0, 9.0), (0, 255, 0), '')], line_width=3, alpha=1.0)
    want = np.ones((10, 12), bool)
    want[2:8, 2:10] = False                                           # lines centred on the border: 2 of their 3 pixels inside
    assert np.array_equal(painted(out, src), want) and out[1, 0, 0] == 255
    far = draw_ref.draw_ref(src, [((-5.0, -5.0, 16.0, 14.0), (0, 255, 0), '')])
    assert np.array_equal(far, src)                                   # the outline lies outside, the interior is not filled


def test_draw_ref_two_overlapping_boxes_in_both_orders():
    src = grey(12, 12)
    a, b = ((1.0, 1.0, 7.0, 7.0), (250, 0, 0), ''), ((4.0, 4.0, 10.0, 10.0), (0, 0, 250), '')
    ab, ba = draw_ref.draw_ref(src, [a, b], alpha=1.0, line_width=1), draw_ref.draw_ref(src, [b, a], alpha=1.0, line_width=1)
    assert ab[:, 4, 7].tolist() == [0, 0, 250] and ba[:, 4, 7].tolist() == [250, 0, 0]       # a crossing: the later box wins
    assert ab[:, 1, 1].tolist() == ba[:, 1, 1].tolist() == [250, 0, 0]
    half = draw_ref.draw_ref(src, [a, b], alpha=0.5, line_width=1)
    once = (128 * 250 + 128 * 100 + 128) >> 8
    assert half[0, 1, 1] == once and half[0, 4, 7] == (128 * 0 + 128 * once + 128) >> 8     # blended twice, in order


def test_draw_ref_tag_geometry_and_ink():
    src = grey(20, 30)
    out = draw_ref.draw_ref(src, [((1.0, 1.0, 28.0, 18.0), (200, 200, 0), '1-')], line_width=1, alpha=1.0)
    tag = out[:, 2:11, 2:15]                                          # at (x1, y1) + line_width, (6 * 2 + 1) x 9 cells
    ink = (tag == 0).all(0)
    one = np.array([[c == '#' for c in r] for r in ('..#..', '.##..', '..#..', '..#..', '..#..', '..#..', '.###.')])
    assert np.array_equal(ink[1:8, 1:6], one) and ink[4, 7:12].all() and int(ink.sum()) == one.sum() + 5
    assert (tag[0][~ink] == 200).all() and (out[2, 2:11, 15] == 100).all() and (out[2, 11, 2:15] == 100).all()
    big = draw_ref.draw_ref(grey(40, 60), [((1.0, 1.0, 28.0, 18.0), (200, 200, 0), '1-', 2)], line_width=1, alpha=1.0)
    assert np.array_equal((big[:, 2:20, 2:28] == 0).all(0), np.kron(ink, np.ones((2, 2), bool)))


def test_font_of_the_kernel_is_the_font_of_the_reference():
    """the glyph bytes in csrc/draw_tracks.hip, read as text, against draw_ref's glyphs"""
    with open(os.path.join(ROOT, 'stereotracking_amd', 'csrc', 'draw_tracks.hip')) as f:
        body = re.search(r'kFont\[14\]\[7\] = \{(.*?)\};', f.read(), re.S).group(1)
    rows = [int(x, 16) for x in re.findall(r'0x[0-9A-Fa-f]{2}', body)]
    assert len(rows) == 14 * 7
    for i, ch in enumerate('0123456789 .|-'):
        want = draw_ref.glyph(ch)
        got = np.array([[(rows[i * 7 + r] >> (4 - c)) & 1 for c in range(5)] for r in range(7)], bool)
        assert np.array_equal(got, want), ch
