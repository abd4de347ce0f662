"""The Kalman filter of the tracker as plain Python floats and loops, in the operation order of
stereotracking_amd/csrc/ocsort_tracker.cpp (kf_initiate / kf_predict / kf_update; csrc/batched_assoc.hip holds the same
loops for the device).  Python floats are IEEE float64, every `*`, `+`, `-`, `/` and math.sqrt below is ONE correctly
rounded operation and nothing is contracted into an FMA - which is what the library's -ffp-contract=off build evaluates.
So a Python-backend tracker driven by `LoopKalmanFilter` as `model.motion` must hold, bit for bit, the state the native
tracker holds (tests/test_cpu_tracker_state.py), and the device tracker's (tests/test_tracker_state_gpu.py).

Spec of the arithmetic: reference mmtrack/models/motion/kalman_filter.py:60-189 (initiate, predict, project, update);
stereotracking_amd/motion.py is its numpy / scipy restatement (LAPACK Cholesky, BLAS products: another operation order).

The interface is motion.KalmanFilter's: initiate(measurement) / predict(mean, cov) / update(mean, cov, measurement) on
numpy arrays, NEW arrays out (the tracker keeps references to the old ones as its `saved` filter).  The constructor's
arguments exist for the perturbed filters of the teeth test only."""
import math

import numpy as np

W_POS = 1.0 / 20
W_VEL = 1.0 / 160


def _div(a, b):
    """IEEE a / b (Python raises on a zero divisor where C returns inf / NaN)."""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)


def _sqrt(x):
    """IEEE sqrt (math.sqrt raises on a negative argument where C returns NaN)."""
    if x != x or x < 0.0:
        return math.nan
    return math.sqrt(x)


def loop_initiate(meas, w_pos=W_POS, w_vel=W_VEL):
    """kf_initiate: (cx, cy, a, h) -> (mean[8], cov[8][8]) as lists of Python floats."""
    mean = [float(meas[i]) for i in range(4)] + [0.0] * 4
    h = float(meas[3])
    std = [2 * w_pos * h, 2 * w_pos * h, 1e-2, 2 * w_pos * h, 10 * w_vel * h, 10 * w_vel * h, 1e-5, 10 * w_vel * h]
    cov = [[0.0] * 8 for _ in range(8)]
    for i in range(8):
        cov[i][i] = std[i] * std[i]
    return mean, cov


def loop_predict(mean, cov, w_pos=W_POS, w_vel=W_VEL, aspect_std=1e-2):
    """kf_predict: mean' = F mean, cov' = F (cov F^T) + Q with F = I + shift(4)."""
    h = mean[3]
    std = [w_pos * h, w_pos * h, aspect_std, w_pos * h, w_vel * h, w_vel * h, 1e-5, w_vel * h]
    new_mean = list(mean)
    for i in range(4):
        new_mean[i] = mean[i] + mean[i + 4]
    t = [[cov[i][j] + cov[i][j + 4] if j < 4 else cov[i][j] for j in range(8)] for i in range(8)]
    new_cov = [[t[i][j] + t[i + 4][j] if i < 4 else t[i][j] for j in range(8)] for i in range(8)]
    for i in range(8):
        new_cov[i][i] = new_cov[i][i] + std[i] * std[i]
    return new_mean, new_cov


def loop_update(mean, cov, meas, w_pos=W_POS):
    """kf_update: project, 4x4 Cholesky, gain^T by two triangular solves per state column, mean and covariance."""
    h = mean[3]
    std = [w_pos * h, w_pos * h, 1e-1, w_pos * h]
    S = [[cov[i][j] + (std[i] * std[i] if i == j else 0.0) for j in range(4)] for i in range(4)]
    L = [[0.0] * 4 for _ in range(4)]
    for j in range(4):
        d = S[j][j]
        for k in range(j):
            d = d - L[j][k] * L[j][k]
        d = _sqrt(d)
        L[j][j] = d
        for i in range(j + 1, 4):
            v = S[i][j]
            for k in range(j):
                v = v - L[i][k] * L[j][k]
            L[i][j] = _div(v, d)
    X = [[0.0] * 8 for _ in range(4)]            # gain^T: solve S X = (cov H^T)^T, B[r][c] = cov[c][r]
    for c in range(8):
        y = [0.0] * 4
        for i in range(4):                       # L y = b
            v = cov[c][i]
            for k in range(i):
                v = v - L[i][k] * y[k]
            y[i] = _div(v, L[i][i])
        for i in range(3, -1, -1):               # L^T x = y
            v = y[i]
            for k in range(i + 1, 4):
                v = v - L[k][i] * X[k][c]
            X[i][c] = _div(v, L[i][i])
    innov = [float(meas[i]) - mean[i] for i in range(4)]
    new_mean = list(mean)
    for c in range(8):
        acc = 0.0
        for r in range(4):
            acc = acc + innov[r] * X[r][c]
        new_mean[c] = mean[c] + acc
    SX = [[0.0] * 8 for _ in range(4)]
    for r in range(4):
        for c in range(8):
            acc = 0.0
            for k in range(4):
                acc = acc + S[r][k] * X[k][c]
            SX[r][c] = acc
    new_cov = [[0.0] * 8 for _ in range(8)]
    for i in range(8):
        for j in range(8):
            acc = 0.0
            for k in range(4):
                acc = acc + X[k][i] * SX[k][j]
            new_cov[i][j] = cov[i][j] - acc
    return new_mean, new_cov


def _lists(mean, cov):
    return [float(v) for v in mean], [[float(v) for v in row] for row in cov]


def _arrays(mean, cov):
    return np.array(mean, np.float64), np.array(cov, np.float64)


class LoopKalmanFilter:
    """motion.KalmanFilter's interface over the loops above."""

    def __init__(self, w_vel=W_VEL, predict_aspect_std=1e-2):
        self.w_pos, self.w_vel, self.predict_aspect_std = W_POS, w_vel, predict_aspect_std

    def initiate(self, measurement):
        return _arrays(*loop_initiate(measurement, self.w_pos, self.w_vel))

    def predict(self, mean, covariance):
        return _arrays(*loop_predict(*_lists(mean, covariance), self.w_pos, self.w_vel, self.predict_aspect_std))

    def update(self, mean, covariance, measurement, bbox_score=0.):
        return _arrays(*loop_update(*_lists(mean, covariance), measurement, self.w_pos))
