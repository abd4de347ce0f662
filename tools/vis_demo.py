#!/usr/bin/env python
"""Paint tracks on frames and write them as JPEG: a visualisation config (default: yolox_s_mmyolo_mot_airdrone_disp_vis.py)
over a tiny synthetic dataset in the AirDrone layout (tools/make_tiny_airdrone.py).  The loop is the test loop in small:
read a frame, model.test_step, then the config's TrackVisualizationHook.after_test_iter with what went in and what came
out - the hook paints on the device (st_draw_tracks) and writes <out>/<frame>.jpg through JpegEncoder (st_jpeg_forward).

Without --checkpoint the detector carries seeded random weights at a reduced width and the tracker's thresholds are
lowered so that it keeps what such a detector finds: the demo shows the overlay path, not the tracker's quality.
usage: python tools/vis_demo.py <data_root> <out_dir> [--config CFG --frames 6 --height 96 --width 160 --score-thr 0.0]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEFAULT_CFG = os.path.join(ROOT, 'configs', 'stereo_tracking', 'ocsort', 'yolox_s_mmyolo_mot_airdrone_disp_vis.py')


def run(config, data_root, out_dir, frames=6, height=96, width=160, device=None, score_thr=None, checkpoint=None, widen=0.375):
    """-> one record per frame: file, height, width, the frame as uint8 (3, H, W) BGR, the boxes the hook painted
    [(xyxy, RGB colour, label)], quality, subsampling."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from make_tiny_airdrone import make
    from stereotracking_amd import datasets as ds, mot, visualization as vis  # noqa: F401
    from stereotracking_amd.config import Config
    from stereotracking_amd.registry import HOOKS, MODELS, VISUALIZERS
    from stereotracking_amd.structures import TrackDataSample
    from stereotracking_amd.synthetic import synthetic_state_dict
    dev = torch.device('cuda:0') if device is None else torch.device(device)
    base, _ = make(data_root, videos=1, frames=frames, height=height, width=width)
    dataset = ds.MOTDispDataset(ann_file='annotations/val_cocoformat_80.json', data_root=base + os.sep,
                                data_prefix=dict(img_path='val/'))
    cfg = Config.fromfile(config)
    if checkpoint is None:
        for part in ('backbone', 'neck'):
            cfg.model.detector[part]['widen_factor'] = widen
        cfg.model.detector.bbox_head.head_module['widen_factor'] = widen
        cfg.model.tracker['init_track_thr'] = 0.03
        cfg.model.tracker['obj_score_thr'] = 0.02
    model = MODELS.build(dict(cfg.model, autotune=False))
    if checkpoint is None:
        model.detector.load_state_dict(synthetic_state_dict(list(model.detector._table), seed=5, prior_prob=0.2, logit_std=2.5),
                                       strict=False)
    else:
        from stereotracking_amd.checkpoint import load_checkpoint
        load_checkpoint(model, checkpoint)
    visualizer = VISUALIZERS.build(cfg.visualizer)
    hook_cfg = dict(cfg.default_hooks.visualization, test_out_dir=out_dir, visualizer=visualizer)
    if score_thr is not None:
        hook_cfg['score_thr'] = score_thr
    hook = HOOKS.build(hook_cfg)
    record = []
    for t in range(len(dataset)):
        info = dataset.get_data_info(t)
        rgb = ds.read_png(info['img_path'])
        codes = np.asarray(ds.read_png(info['disp_path'])).astype(np.float32)
        disp = np.where(codes == 65535, 0.0, codes / 16.0).astype(np.float32)           # loading_disparity.py:82,129-134
        bgr = np.ascontiguousarray(rgb[..., ::-1].transpose(2, 0, 1))
        img = torch.from_numpy(bgr)[None].to(dev)
        disp_t = torch.from_numpy(disp)[None, None].repeat(1, 3, 1, 1)
        sample = TrackDataSample(dict(frame_id=info['frame_id'], ori_shape=(height, width), img_shape=(height, width),
                                      scale_factor=(1.0, 1.0), img_path=info['img_path']))
        batch = dict(inputs=dict(img=[img], disp_postp=[disp_t], disp_mask=[(disp_t[:, :1] > 0).to(torch.uint8)]),
                     data_samples=[sample])
        outs = model.test_step(batch)
        files = hook.after_test_iter(None, t, batch, outs)
        pred = outs[0].pred_track_instances
        if 'scores' in pred:
            pred = pred[pred.scores > hook.score_thr]
        record.append(dict(file=files[0], height=height, width=width, frame_bgr=bgr, boxes=vis.instance_boxes(pred),
                           quality=visualizer.quality, subsampling=visualizer.subsampling))
    torch.cuda.synchronize()
    visualizer.close()
    return record


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('data_root')
    ap.add_argument('out_dir')
    ap.add_argument('--config', default=DEFAULT_CFG)
    ap.add_argument('--frames', type=int, default=6)
    ap.add_argument('--height', type=int, default=96)
    ap.add_argument('--width', type=int, default=160)
    ap.add_argument('--score-thr', type=float, default=0.0, help='the hook\'s threshold (random weights score low)')
    ap.add_argument('--checkpoint', default=None)
    a = ap.parse_args()
    record = run(a.config, a.data_root, a.out_dir, a.frames, a.height, a.width, score_thr=a.score_thr, checkpoint=a.checkpoint)
    for r in record:
        print(f"{r['file']}: {len(r['boxes'])} boxes")


if __name__ == '__main__':
    main()
