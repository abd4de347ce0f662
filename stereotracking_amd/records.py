"""Column layouts of the float records that carry detections and tracks from the device to the result containers, and
the builders of those containers.

  frame record   pipeline.pack_detections: (M + 1, 8) or, scaled='both', (M + 1, 13) float32.  Row REC_HEADER =
                 [detections kept (true count, may exceed M), M, valid-frame flag, 0...]; rows 1..M = [box, score, label,
                 depth, scale] + [depth-scaled box, kept prior index] in the 13-column form
  track row      the native tracker's output, 8 floats: a frame record's first 8 columns
  stream tick    include/stereotrack.h (st_stream_record): per stream STREAM_HDR_INTS int32 [track rows, detections kept,
                 tracker status, frame id], track rows [box, score, label, scale, depth, gt depth, 0] and detection rows
                 [box, score, label, kept prior index, 0]
Depth and scale swap places between the native track row and the stream tick's: TRACK_ROW / STREAM_ROW say which."""
from collections import namedtuple

import numpy as np
import torch

from .structures import InstanceData

BOX, SCORE, LABEL = slice(0, 4), 4, 5                  # the first six columns of every row layout above
REC_HEADER, REC_COUNT, REC_CAP = 0, 0, 1               # frame record: the header row and its first two columns
REC_VALID = 2                                          # header row: the valid-frame flag (0 = batch padding, not a frame)
REC_FLOATS, REC_FLOATS_BOTH = 8, 13
REC_DEPTH, REC_SCALE, REC_SCALED_BOX, REC_PRIOR = 6, 7, slice(8, 12), 12
TrackLayout = namedtuple('TrackLayout', 'floats depth scale gt_depth')
TRACK_ROW = TrackLayout(REC_FLOATS, REC_DEPTH, REC_SCALE, None)
STREAM_ROW = TrackLayout(10, 7, 6, 8)                  # ST_STREAM_ROW_FLOATS
STREAM_HDR_INTS, STREAM_DET_FLOATS, STREAM_DET_PRIOR = 4, 8, 6     # ST_STREAM_HDR_INTS / ST_STREAM_DET_FLOATS


def int_column(rows, col):
    """Column `col` of float32 numpy rows (..., C) -> int64 tensor of its own (labels, prior indices)."""
    return torch.from_numpy(rows[..., col].astype(np.int64))


def detections(rows, labels, prior_idx):
    """pred_det_instances of a result (reference ocsort_disparity.py:107-108): boxes and scores are VIEWS of the
    detection rows (k, C) - the caller copies a page-locked buffer first -, labels / prior_idx come from int_column."""
    return InstanceData(bboxes=rows[:, BOX], scores=rows[:, SCORE], labels=labels, prior_idx=prior_idx)


def tracks(rows, labels, ids, layout):
    """pred_track_instances from track rows (m, layout.floats) + ids (m,): views of `rows`; the stream tick's completed
    rows yield depth / gt_depth as tensors of their own, like the shell's finish() writes them."""
    out = InstanceData()
    out['bboxes'] = rows[:, BOX]
    out['labels'] = labels
    out['scores'] = rows[:, SCORE]
    out['scales'] = rows[:, layout.scale]
    depth = rows[:, layout.depth]
    out['depth'] = depth if layout.gt_depth is None else depth.clone()
    if layout.gt_depth is not None:
        out['gt_depth'] = rows[:, layout.gt_depth].clone()
    out.instances_id = ids
    return out
