"""Generates tests/golden/gsi_truth.npz: the fixture of the Gaussian-smoothed interpolation tests.

Run once on a machine with mpmath and scikit-learn (`python tests/golden/make_gsi_golden.py`, and again with `--long`
for tests/golden/gsi_truth_long.npz: one 512-row track in the same format); the tests read only the .npz files.  Per case it stores the track (frames, the four coordinate columns, smooth_tau, len_scale) and
  truth    K (K + 1e-10 I)^-1 y evaluated with mpmath at 60 digits (one LU factorisation, four right-hand sides),
           rounded to fp64: the yardstick, because the system is ill-conditioned by design and any two correct fp64
           evaluations differ at 1e-5 .. 1e-4 px;
  sklearn  GaussianProcessRegressor(RBF(len_scale, 'fixed')).fit(t, y).predict(t), what the reference calls;
  ref_err  max |sklearn - truth|, the scale of the tests' tolerance.
Every gap of the stored frame lists is 1 or >= 20 frames, so InterpolateTracklets(max_num_frames=20) fills nothing and
the track that reaches the smoother is the stored one.
"""
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ALPHA = 1e-10


def len_scale_of(tau, n):
    return float(np.clip(tau * np.log(tau ** 3 / n), tau ** -1, tau ** 2))


def path(frames, seed, noise=2.5):
    """A smooth path through about 600 .. 1900 px with `noise` px of normal noise: x1, y1, x2, y2."""
    rng = np.random.default_rng(seed)
    t = frames.astype(np.float64)
    s = (t - t[0]) / max(1.0, t[-1] - t[0])
    x1 = 620.0 + 900.0 * s + 60.0 * np.sin(4.0 * s + 0.3 * seed)
    y1 = 700.0 + 500.0 * s * s + 40.0 * np.cos(5.0 * s)
    w = 180.0 + 60.0 * s
    h = 240.0 - 50.0 * s
    y = np.stack([x1, y1, x1 + w, y1 + h])
    return y + noise * rng.standard_normal(y.shape)


def cases():
    def run(n, start=0):
        return np.arange(start, start + n, dtype=np.int64)
    out = [('n3', run(3, 7), 10), ('n10_gaps', np.array([3, 4, 5, 30, 31, 61, 62, 63, 64, 90], np.int64), 10)]
    # 63 / 64 / 65: a tile edge of the trailing update; 127 / 128 / 129: the matrix leaves LDS for the global workspace
    # above 128 rows; 255 / 256 / 257: a thread owns a second row above 256
    for n in (63, 64, 65, 127, 128, 129, 255, 257):
        out.append((f'n{n}', run(n, 1), 10))
    out.append(('n77_tau20', run(77, 1), 20))
    out.append(('tau1_n40', run(40, 1), 1))
    out.append(('tau4_n70', run(70, 1), 4))
    out.append(('linear64', run(64, 1), 10))
    out.append(('n256_gap25', np.concatenate([run(100, 1), run(156, 125)]), 10))
    return out


def solve_case(arg):
    i, (name, frames, tau) = arg
    import mpmath as mp
    from sklearn.gaussian_process import GaussianProcessRegressor as GPR
    from sklearn.gaussian_process.kernels import RBF
    n = len(frames)
    ls = len_scale_of(tau, n)
    if name == 'linear64':
        t = frames.astype(np.float64)
        y = np.stack([600.0 + 2.5 * t, 900.0 - 1.25 * t, 800.0 + 3.0 * t, 1200.0 - 0.5 * t])   # exact in fp64
    else:
        y = path(frames, seed=100 + i)
    mp.mp.dps = 60
    tf = [mp.mpf(int(v)) for v in frames]
    lsm = mp.mpf(ls)
    K = mp.matrix(n, n)
    for a in range(n):
        for b in range(a + 1):
            v = mp.exp(-((tf[a] - tf[b]) / lsm) ** 2 / 2)
            K[a, b] = v
            K[b, a] = v
    A = K.copy()
    for a in range(n):
        A[a, a] += mp.mpf(ALPHA)
    LU, p = mp.mp.LU_decomp(A)
    truth = np.zeros((4, n))
    for c in range(4):
        col = mp.matrix([mp.mpf(float(v)) for v in y[c]])
        x = mp.mp.U_solve(LU, mp.mp.L_solve(LU, col, p))
        m = K * x
        truth[c] = [float(m[a]) for a in range(n)]
    t2 = frames.astype(np.float64).reshape(-1, 1)
    sk = np.zeros((4, n))
    for c in range(4):
        gpr = GPR(RBF(ls, 'fixed'))
        gpr.fit(t2, y[c].reshape(-1, 1))
        sk[c] = np.asarray(gpr.predict(t2)).reshape(-1)
    return name, frames, tau, ls, y, truth, sk, float(np.abs(sk - truth).max())


def long_cases():
    """The longest track the device smoother takes (512 rows: its global-workspace path at its largest, two rows per
    thread throughout).  About ten minutes of mpmath, so it is kept out of the main fixture, whose cases stop at 260 rows."""
    return [(20, ('n512', np.arange(1, 513, dtype=np.int64), 10))]


def main():
    out = {}
    names = []
    long = '--long' in sys.argv[1:]
    todo, target = (long_cases(), 'gsi_truth_long.npz') if long else (list(enumerate(cases())), 'gsi_truth.npz')
    with ProcessPoolExecutor(max_workers=8) as ex:
        for name, frames, tau, ls, y, truth, sk, err in ex.map(solve_case, todo):
            names.append(name)
            out[name + '/frames'], out[name + '/y'], out[name + '/truth'], out[name + '/sklearn'] = frames, y, truth, sk
            out[name + '/tau'], out[name + '/len_scale'], out[name + '/ref_err'] = np.int64(tau), np.float64(ls), np.float64(err)
            print(f'{name}: n {len(frames)} tau {tau} len_scale {ls:.6g} ref_err {err:.3e}', flush=True)
    out['names'] = np.array(names)
    np.savez_compressed(os.path.join(HERE, target), **out)


if __name__ == '__main__':
    sys.exit(main())
