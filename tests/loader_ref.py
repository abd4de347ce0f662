"""numpy restatement of the reference's disparity loader step, LoadDisparityFromFile._post_processing_v2
(loading_disparity.py:129-134), shared by tests/test_stereo_depth_gpu.py::test_pack_raw_inputs_matches_reference_pipeline
(the yardstick of st_pack_raw_inputs) and tests/test_cpu_reference_fixtures.py (which holds it to the recorded output)."""
import numpy as np


def post_processing_v2(code):
    """uint16 PNG codes -> float32 disparity: the invalid code 65535 -> 0, everything / 16."""
    disp = code.astype(np.float32)
    disp[code == 65535] = 0
    return disp / 16.
