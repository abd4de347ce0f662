"""CameraMotionCompensation: the reference's registered ECC utility (mmtrack/models/motion/
camera_motion_compensation.py), with cv2.findTransformECC replaced by the device estimate of csrc/cmc_ecc.hip.

  get_warp_matrix(img, ref_img)   camera_motion_compensation.py:29-41.  RGB HWC images; template = img, input =
                                  ref_img; full resolution, gaussFiltSize 1 - as the reference calls cv2.  The warp maps
                                  `img` coordinates to `ref_img` coordinates.  cv2 raises where the iteration fails
                                  (no overlap, a flat image, a diverging step); so does this: RuntimeError.
  warp_bboxes(bboxes, warp)       :43-53, the reference's arithmetic.
  track()                         :55-79 works on the reference's Tracktor track containers, which this package does
                                  not have; it stays out.
The rules of the estimate and its stated deviations from cv2: tests/ecc_ref.py, DESIGN.md "ECC camera-motion
compensation".
"""
import numpy as np
import torch

from . import cmc as _cmc
from .registry import TASK_UTILS


@TASK_UTILS.register_module(name=['CameraMotionCompensation', 'mmtrack.CameraMotionCompensation'])
class CameraMotionCompensation:
    def __init__(self, warp_mode='cv2.MOTION_EUCLIDEAN', num_iters=50, stop_eps=0.001):
        self.params = _cmc.ecc_params(dict(warp_mode=warp_mode, num_iters=num_iters, stop_eps=stop_eps,
                                           gauss_filt_size=1, downscale=1))
        self.warp_mode = self.params['warp_mode']
        self.num_iters = self.params['num_iters']
        self.stop_eps = self.params['stop_eps']

    @staticmethod
    def _bgr_chw(img, dev):
        """RGB (h, w, 3) array / tensor -> uint8 (1, 3, h, w) BGR frame on the device, the form the front takes."""
        t = torch.as_tensor(np.ascontiguousarray(img)) if isinstance(img, np.ndarray) else img
        if t.dim() != 3 or t.shape[2] != 3:
            raise ValueError('CameraMotionCompensation: images must be RGB (h, w, 3)')
        if t.dtype != torch.uint8:
            t = t.clamp(0, 255).to(torch.uint8)
        return t.to(dev).flip(2).permute(2, 0, 1)[None].contiguous()

    def get_warp_matrix(self, img, ref_img):
        dev = next((t.device for t in (img, ref_img) if isinstance(t, torch.Tensor) and t.is_cuda), None)
        if dev is None:
            dev = torch.device('cuda', torch.cuda.current_device())
        a, b = self._bgr_chw(img, dev), self._bgr_chw(ref_img, dev)
        if a.shape != b.shape:
            raise ValueError('CameraMotionCompensation: img and ref_img differ in size')
        h, w = int(a.shape[2]), int(a.shape[3])
        planes = _cmc.ecc_front([a, b], h, w, 1)
        row = _cmc.ecc_estimate(planes[0:1], planes[1:2], h, w, self.params)[0].cpu()
        if float(row[0]) == 0:
            raise RuntimeError('CameraMotionCompensation: the ECC iteration failed (no overlap, a flat image, or the '
                               'correlation would decrease); cv2.findTransformECC raises there')
        return row[2:8].reshape(2, 3).clone()

    def warp_bboxes(self, bboxes, warp_matrix):
        """(K, 4) xyxy boxes -> both corners of every box moved by the 2 x 3 warp: corner' = warp (x, y, 1)."""
        corners = bboxes.reshape(-1, 2)                                   # top-left, bottom-right of box 0, of box 1, ...
        homog = torch.cat((corners, corners.new_ones(corners.shape[0], 1)), dim=1)
        return torch.mm(homog, warp_matrix.to(bboxes).t()).reshape(-1, 4)
