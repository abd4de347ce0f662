// The OC-SORT core: the ONE copy of everything the host tracker (ocsort_tracker.cpp, st_tracker_track*) and the device
// tracker (batched_assoc.hip; the unscale kernel of stream_track.hip) must agree on to the bit - the float64 Kalman
// filter, the float32 box helpers, the observation history and the feeding of a track, the entry of a stage's cost
// matrix, the two predicates "a detection enters association" / "a track is dropped", and the unscale of a returned row.  Both trackers are built by the same
// rule with the same flags (-ffp-contract=off), so one __host__ __device__ text gives both the same single IEEE
// operations in the same order.  What stays with each tracker is what only it has: the stage driver, the assignment and
// the cost loop on either side, camera motion on the host, the wave-cooperative driver on the device.
//
// The routines that touch a track are templates over the track type: DTrack (fixed window, the device's record) and
// Track (window sized at creation, the host's).  Also a plain C++ header: tests/native/ocsort_core_check.cpp drives both
// track types through it on the CPU under sanitizers, without HIP.
//
// Behavioural spec (file:line in the reference):
//   KalmanFilter initiate / predict / project / update         mmtrack/models/motion/kalman_filter.py:38-189
//   init_track / update_track                                  mmtrack/models/trackers/ocsort_tracker_disparity.py:105-146
//   vel_direction, k_step_observation, online_smooth           :148-156, :173-185, :319-343
#pragma once
#include <array>
#include <cmath>
#include <cstdint>
#include <vector>

#ifdef __HIPCC__
#define ST_OC_HD __host__ __device__
#else
#define ST_OC_HD
#endif

namespace st {
namespace oc {

constexpr int WINCAP = 8;           // DTrack: vel_delta_t + 1 <= 8 observations kept per track
constexpr double kWPos = 1.0 / 20, kWVel = 1.0 / 160;

struct KState { double mean[8]; double cov[64]; };

// The device's track record.  The kernels move it as 8-byte words and st_batched_tracker_get_states reads it: size and
// field order are fixed.
struct DTrack {
  long long id;
  KState kf, saved;
  int tentative, tracked, last_frame, n_fed;
  float win[WINCAP][4];
  int win_valid[WINCAP];
  int win_len;
  long long n_obs;
  float last_valid[4];
  int trailing_none;
  float vel[2];
  int vel_placeholder;
};

// The host's track: the same fields, the window's storage sized vel_delta_t + 1 at creation (any vel_delta_t >= 0).
struct Track {
  explicit Track(int vel_delta_t) : win((size_t)vel_delta_t + 1), win_valid((size_t)vel_delta_t + 1) {}
  int64_t id = 0;
  KState kf{}, saved{};
  bool tentative = true, tracked = true;
  int last_frame = 0;
  int n_fed = 0;                 // len(track.bboxes): frames this track was fed a detection
  // observation history (track.obs): only what the algorithm reads back is kept -
  //   the last vel_delta_t + 1 entries (k_step_observation), the last non-None entry and the trailing None count
  std::vector<std::array<float, 4>> win;   // the most recent entries, oldest at index 0; [0, win_len) are in use
  std::vector<char> win_valid;
  int win_len = 0;
  long long n_obs = 0;
  float last_valid[4] = {0.f, 0.f, 0.f, 0.f};
  int trailing_none = 0;
  float vel[2] = {-1.f, -1.f};
  bool vel_placeholder = true;   // velocity == tensor((-1, -1)) (sum == -2 -> "no velocity yet")
};

// ---- Kalman filter (kalman_filter.py:38-189), float64 -----------------------------------------------------------------
ST_OC_HD inline void kf_initiate(const float meas[4], KState& s) {
  for (int i = 0; i < 4; ++i) { s.mean[i] = (double)meas[i]; s.mean[4 + i] = 0.0; }
  const double h = (double)meas[3];
  const double sd[8] = {2 * kWPos * h, 2 * kWPos * h, 1e-2, 2 * kWPos * h,
                        10 * kWVel * h, 10 * kWVel * h, 1e-5, 10 * kWVel * h};
  for (int i = 0; i < 64; ++i) s.cov[i] = 0.0;
  for (int i = 0; i < 8; ++i) s.cov[i * 8 + i] = sd[i] * sd[i];
}

ST_OC_HD inline void kf_predict(KState& s) {
  const double h = s.mean[3];
  const double sd[8] = {kWPos * h, kWPos * h, 1e-2, kWPos * h, kWVel * h, kWVel * h, 1e-5, kWVel * h};
  // mean' = F mean : F = I + shift(4): rows < 4 add the velocity
  for (int i = 0; i < 4; ++i) s.mean[i] = s.mean[i] + s.mean[i + 4];
  // cov' = F (cov F^T) + Q   (numpy multi_dot picks A(BC) when both orders cost the same)
  double t[64];
  for (int i = 0; i < 8; ++i)
    for (int j = 0; j < 8; ++j) t[i * 8 + j] = j < 4 ? s.cov[i * 8 + j] + s.cov[i * 8 + j + 4] : s.cov[i * 8 + j];
  for (int i = 0; i < 8; ++i)
    for (int j = 0; j < 8; ++j) s.cov[i * 8 + j] = i < 4 ? t[i * 8 + j] + t[(i + 4) * 8 + j] : t[i * 8 + j];
  for (int i = 0; i < 8; ++i) s.cov[i * 8 + i] += sd[i] * sd[i];
}

ST_OC_HD inline void kf_update(KState& s, const float meas[4]) {
  // project: mean_p = mean[:4], S = cov[:4,:4] + diag(std^2)
  const double h = s.mean[3];
  const double sd[4] = {kWPos * h, kWPos * h, 1e-1, kWPos * h};
  double S[16];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) S[i * 4 + j] = s.cov[i * 8 + j] + (i == j ? sd[i] * sd[i] : 0.0);
  // Cholesky S = L L^T (lower)
  double L[16];
  for (int i = 0; i < 16; ++i) L[i] = 0.0;
  for (int j = 0; j < 4; ++j) {
    double d = S[j * 4 + j];
    for (int k = 0; k < j; ++k) d -= L[j * 4 + k] * L[j * 4 + k];
    d = std::sqrt(d);
    L[j * 4 + j] = d;
    for (int i = j + 1; i < 4; ++i) {
      double v = S[i * 4 + j];
      for (int k = 0; k < j; ++k) v -= L[i * 4 + k] * L[j * 4 + k];
      L[i * 4 + j] = v / d;
    }
  }
  // gain^T = S^-1 (cov H^T)^T : solve S X = B with B[r][c] = cov[c][r] (4 x 8), X = gain^T
  double X[32];
  for (int c = 0; c < 8; ++c) {
    double y[4];
    for (int i = 0; i < 4; ++i) {      // L y = b
      double v = s.cov[c * 8 + i];
      for (int k = 0; k < i; ++k) v -= L[i * 4 + k] * y[k];
      y[i] = v / L[i * 4 + i];
    }
    for (int i = 3; i >= 0; --i) {     // L^T x = y
      double v = y[i];
      for (int k = i + 1; k < 4; ++k) v -= L[k * 4 + i] * X[k * 8 + c];
      X[i * 8 + c] = v / L[i * 4 + i];
    }
  }
  double innov[4];
  for (int i = 0; i < 4; ++i) innov[i] = (double)meas[i] - s.mean[i];
  // new_mean = mean + innovation . gain^T
  for (int c = 0; c < 8; ++c) {
    double acc = 0.0;
    for (int r = 0; r < 4; ++r) acc += innov[r] * X[r * 8 + c];
    s.mean[c] += acc;
  }
  // new_cov = cov - gain (S gain^T)
  double SX[32];
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 8; ++c) {
      double acc = 0.0;
      for (int k = 0; k < 4; ++k) acc += S[r * 4 + k] * X[k * 8 + c];
      SX[r * 8 + c] = acc;
    }
  for (int i = 0; i < 8; ++i)
    for (int j = 0; j < 8; ++j) {
      double acc = 0.0;
      for (int k = 0; k < 4; ++k) acc += X[k * 8 + i] * SX[k * 8 + j];
      s.cov[i * 8 + j] -= acc;
    }
}

// ---- float32 box helpers (single IEEE ops, reference order) -----------------------------------------------------------
ST_OC_HD inline void xyxy_to_cxcyah(const float b[4], float o[4]) {   // structures/bbox/transforms.py:72-86
  o[0] = (b[2] + b[0]) / 2;
  o[1] = (b[3] + b[1]) / 2;
  const float w = b[2] - b[0], h = b[3] - b[1];
  o[2] = w / h;
  o[3] = h;
}

ST_OC_HD inline void cxcyah_to_xyxy(const float b[4], float o[4]) {   // transforms.py:89-101
  const float w = b[2] * b[3];
  o[0] = b[0] - w / 2.0f;
  o[1] = b[1] - b[3] / 2.0f;
  o[2] = b[0] + w / 2.0f;
  o[3] = b[1] + b[3] / 2.0f;
}

// torch.max / torch.min / clamp propagate NaN (std::fmax would drop it): a NaN box must give a NaN cost
ST_OC_HD inline float tmax(float a, float b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }
ST_OC_HD inline float tmin(float a, float b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }

ST_OC_HD inline float iou(const float a[4], const float b[4]) {       // mmdet bbox_overlaps, mode='iou', eps 1e-6
  const float area1 = (a[2] - a[0]) * (a[3] - a[1]);
  const float area2 = (b[2] - b[0]) * (b[3] - b[1]);
  const float w = tmax(tmin(a[2], b[2]) - tmax(a[0], b[0]), 0.f);   // (rb - lt).clamp(min=0)
  const float h = tmax(tmin(a[3], b[3]) - tmax(a[1], b[1]), 0.f);
  const float overlap = w * h;
  const float uni = tmax(area1 + area2 - overlap, 1e-6f);           // torch.max(union, eps)
  return overlap / uni;
}

// scale_bbox(track box, 1 / scale) of a returned row (x1, y1, x2, y2, score, label, depth, scale) -> out[0..4)
// (ocsort_disparity.py:95-97, trackers/utils.py:58-73) as the same fp32 single operations torch evaluates.  Every read
// of the row precedes the first write: out may be the row itself.
ST_OC_HD inline void unscale_box(const float* r, float* out) {
  const float inv = 1.0f / r[7];
  const float cx = (r[0] + r[2]) / 2.0f, cy = (r[1] + r[3]) / 2.0f;
  const float w = (r[2] - r[0]) * inv, h = (r[3] - r[1]) * inv;
  out[0] = cx - w / 2.0f; out[1] = cy - h / 2.0f; out[2] = cx + w / 2.0f; out[3] = cy + h / 2.0f;
}

// One entry of a stage's cost matrix: tb = the track's box (OCM: Kalman-predicted; OCR: last observation), d = the
// detection row.  with_motion (OCM) adds the velocity-direction term (:187-265): ko = the track's k-step-old observation,
// vel = its velocity direction, valid = that direction is one.
ST_OC_HD inline float cost_entry(const float tb[4], const float* d, bool with_motion, const float* ko, const float* vel,
                                 bool valid, int weight_iou_with_det_scores, float vel_consist_weight) {
  float v = iou(tb, d);
  if (weight_iou_with_det_scores) v = v * d[4];
  float dist = 1.0f - v;
  if (with_motion) {
    // direction from the k-step-old observation to this detection vs the track's velocity direction
    const float cx1 = (ko[0] + ko[2]) / 2.0f, cy1 = (ko[1] + ko[3]) / 2.0f;
    const float cx2 = (d[0] + d[2]) / 2.0f, cy2 = (d[1] + d[3]) / 2.0f;
    const float sy = cy2 - cy1, sx = cx2 - cx1;
    const float norm = std::sqrt(sy * sy + sx * sx) + 1e-6f;
    float cosv = (sy / norm) * vel[0] + (sx / norm) * vel[1];
    cosv = cosv < -1.f ? -1.f : (cosv > 1.f ? 1.f : cosv);
    const float ang = (std::acos(cosv) - (float)(M_PI / 2.)) / (float)M_PI;
    const float term = ang * (valid ? 1.0f : 0.0f);
    dist = dist + term * vel_consist_weight;
  }
  return dist;
}

// ---- predicates --------------------------------------------------------------------------------------------------------
// a detection row enters association (ocsort_tracker_disparity.py:409-421)
ST_OC_HD inline bool enters_association(const float* d, float obj_score_thr) {
  const float area = (d[2] - d[0]) * (d[3] - d[1]);
  return d[4] > obj_score_thr && area > 100.f;
}
// KalmanTrackerBase.pop_invalid_tracks (kalman_tracker_base.py:78-88).  The track comes by pointer: a reference
// parameter is marked dereferenceable, the compiler then reads `tentative` ahead of the first test, and the device
// kernels' code (register allocation throughout) is no longer the code of the expression written in place.
template <class T>
ST_OC_HD inline bool is_dropped(const T* t, int frame_id, int num_frames_retain) {
  return frame_id - t->last_frame >= num_frames_retain || (t->tentative && t->last_frame != frame_id);
}

// ---- observation history and the feeding of a track --------------------------------------------------------------------
// box == nullptr: the track was not matched in this frame (a None entry of track.obs)
template <class T>
ST_OC_HD inline void push_obs(T& t, const float* box, int vel_delta_t) {
  const int cap = vel_delta_t + 1;
  if (t.win_len == cap) {
    for (int k = 1; k < cap; ++k) {
      for (int e = 0; e < 4; ++e) t.win[k - 1][e] = t.win[k][e];
      t.win_valid[k - 1] = t.win_valid[k];
    }
    --t.win_len;
  }
  for (int e = 0; e < 4; ++e) t.win[t.win_len][e] = box ? box[e] : 0.f;
  t.win_valid[t.win_len] = box != nullptr;
  ++t.win_len;
  ++t.n_obs;
  if (box) {
    for (int e = 0; e < 4; ++e) t.last_valid[e] = box[e];
    t.trailing_none = 0;
  } else {
    ++t.trailing_none;
  }
}
// obs[num_obs - 1 - vel_delta_t] when it exists and is a detection, else the last detection (:173-185)
template <class T>
ST_OC_HD inline const float* k_step_observation(const T& t, int vel_delta_t) {
  if (t.n_obs > vel_delta_t && t.win_len == vel_delta_t + 1 && t.win_valid[0]) return &t.win[0][0];
  return t.last_valid;
}
template <class T>
ST_OC_HD inline void set_velocity(T& t, const float* b1, const float* b2) {   // vel_direction (:148-156)
  const float s1 = ((b1[0] + b1[1]) + b1[2]) + b1[3], s2 = ((b2[0] + b2[1]) + b2[2]) + b2[3];
  if (s1 < 0 || s2 < 0) { t.vel[0] = t.vel[1] = -1.f; t.vel_placeholder = 1; return; }
  const float cx1 = (b1[0] + b1[2]) / 2.0f, cy1 = (b1[1] + b1[3]) / 2.0f;
  const float cx2 = (b2[0] + b2[2]) / 2.0f, cy2 = (b2[1] + b2[3]) / 2.0f;
  const float sy = cy2 - cy1, sx = cx2 - cx1;
  const float norm = std::sqrt(sy * sy + sx * sx) + 1e-6f;
  t.vel[0] = sy / norm;
  t.vel[1] = sx / norm;
  t.vel_placeholder = (t.vel[0] + t.vel[1]) == -2.0f;
}
// every field of t is written (the device reuses a dropped track's slot)
template <class T>
ST_OC_HD inline void init_track(T& t, long long id, const float* row, int frame_id, int vel_delta_t) {
  t.id = id;
  t.n_fed = 1;
  t.last_frame = frame_id;
  t.tentative = frame_id != 0;        // tracks born on frame 0 are confirmed at once (:108-111)
  t.win_len = 0;
  t.n_obs = 0;
  t.trailing_none = 0;
  for (int e = 0; e < 4; ++e) t.last_valid[e] = 0.f;
  t.vel[0] = t.vel[1] = -1.f;
  t.vel_placeholder = 1;
  float m[4];
  xyxy_to_cxcyah(row, m);
  kf_initiate(m, t.kf);
  // no saved filter yet (the reference's track has no such item until its first predict as a tracked, confirmed
  // track): zero on both trackers, so that their states compare equal
  for (int i = 0; i < 8; ++i) t.saved.mean[i] = 0.0;
  for (int i = 0; i < 64; ++i) t.saved.cov[i] = 0.0;
  push_obs(t, row, vel_delta_t);
  t.tracked = 1;
}
template <class T>
ST_OC_HD inline void update_track(T& t, const float* row, int frame_id, int num_tentatives, int vel_delta_t) {
  ++t.n_fed;
  t.last_frame = frame_id;
  if (t.tentative && t.n_fed >= num_tentatives) t.tentative = 0;
  float m[4];
  xyxy_to_cxcyah(row, m);
  kf_update(t.kf, m);
  t.tracked = 1;
  push_obs(t, row, vel_delta_t);
  set_velocity(t, k_step_observation(t, vel_delta_t), row);
}
// a re-found track: the Kalman filter restarts from the saved one and is fed the gap's interpolated boxes (:319-343)
template <class T>
ST_OC_HD inline void online_smooth(T& t, const float* new_box) {
  float last[4];
  for (int i = 0; i < 4; ++i) last[i] = t.last_valid[i];
  const int gap = t.trailing_none;
  float step[4];
  for (int i = 0; i < 4; ++i) step[i] = (new_box[i] - last[i]) / (float)(gap + 1);
  t.kf = t.saved;
  for (int g = 0; g < gap; ++g) {
    float vb[4], m[4];
    for (int i = 0; i < 4; ++i) vb[i] = last[i] + (float)(g + 1) * step[i];
    xyxy_to_cxcyah(vb, m);
    kf_update(t.kf, m);
  }
}

}  // namespace oc
}  // namespace st
