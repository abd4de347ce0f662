// Depth-guided OC-SORT association step as a host-side native routine (north_star keeps this step on the CPU).
//
// Behavioural spec (file:line in /root/reference), the same one stereotracking_amd/trackers.py follows in Python:
//   OCSORTTracker_Disparity.track            mmtrack/models/trackers/ocsort_tracker_disparity.py:345-618
//     init_track / update_track              :105-146  (+ kalman_tracker_base.py:55-76, base_tracker.py:54-141)
//     vel_direction(_batch), k_step_observation, last_obs      :148-185, :267-271
//     ocm_assign_ids / ocr_assign_ids / online_smooth          :187-265, :273-317, :319-343
//   KalmanTrackerBase.pop_invalid_tracks     kalman_tracker_base.py:78-88
//   KalmanFilter initiate/predict/project/update               mmtrack/models/motion/kalman_filter.py:60-189
//   lap.lapjv                                -> st_lapjv_extended (lapjv.cpp)
// The Kalman filter, the box helpers, the observation history, the feeding of a track and the cost entry live in
// ocsort_core.h, the one text this file and the device tracker (batched_assoc.hip) both compile; what is here is the
// stage driver track(), camera motion (apply_warp) and track_records, which only the host has.
//
// Why native: the dense path delivers a frame every ~0.75 ms per GPU; the Python tracker (a few hundred tiny
// torch / numpy calls per frame) needs 1-3 ms per frame on 6 objects and would be the bottleneck of
// BASELINE configs[2]/[3].  This routine does the same arithmetic in ~10-20 us.
//
// Numerics.  Everything that DECIDES an assignment is computed in the reference's precision and operation order:
// box conversions, IoU, the velocity-direction term and the cost matrix in float32 (single IEEE operations, file
// compiled with -ffp-contract=off), the assignment in float64 by the same Jonker-Volgenant procedure.  Two things
// can differ from the Python stack in the last bit and are documented rather than hidden: acosf (glibc vs the SLEEF
// routine behind torch.acos: <= 1 ulp, i.e. <= 1e-8 on a cost) and the 4x4 Cholesky / 8x8 products of the Kalman
// update (plain loops here, LAPACK / BLAS there: ~1e-16 relative on the state, invisible after the float32 cast
// the cost matrix applies).  A third, found by the state tests: sqrtf here is correctly rounded, torch.sqrt on the CPU is
// not (1 ulp off on ~0.5 % of inputs); the Python backend takes the root of the STORED velocity direction through
// float64 so that the states agree on the bits, the root inside its cost matrix stays torch's (<= 1 ulp on the
// direction term, like acosf).  Exact ties (duplicate boxes) stay exact ties, because both sides of a tie go through
// identical instructions.  tests/test_cpu_tracker_oracle.py holds the ids, boxes, scores, depth and scales of
// every frame EQUAL to the oracle's and the Kalman state equal to 1e-9.  tests/test_cpu_tracker_state.py holds the
// WHOLE per-track state (st_tracker_get_states) bit-equal to the Python backend driven by these very loops restated
// in Python floats (tests/kalman_ref.py), and those loops to mpmath within 4 x the error of the numpy filter.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "ocsort_core.h"
#include "st_common.h"

extern "C" int st_lapjv_extended(const double* cost, int n_rows, int n_cols, double cost_limit, int32_t* x_out,
                                 int32_t* y_out);

using namespace st::oc;   // Track, the Kalman filter, the box helpers and the routines that feed a track: ocsort_core.h

struct StTracker {
  StTrackerConfig cfg{};
  std::vector<Track> tracks;     // dict insertion order
  long long num_tracks = 0;

  void reset() { tracks.clear(); num_tracks = 0; }
  int find(int64_t id) const {
    for (size_t i = 0; i < tracks.size(); ++i)
      if (tracks[i].id == id) return (int)i;
    return -1;
  }

  // cost matrix of one association stage + assignment; rows = tracks `tidx`, cols = detections `didx`.
  // with_motion: OCM (KF-predicted boxes + velocity-direction term); else OCR (last observations, IoU only).
  // The device's form of this loop, an entry per lane, is assign_stage (batched_assoc.hip).
  void assign(const std::vector<int>& tidx, const std::vector<int>& didx, const float* dets, bool with_motion,
              std::vector<int32_t>& det_to_row) {
    const int R = (int)tidx.size(), Cn = (int)didx.size();
    det_to_row.assign(Cn, -1);
    if (R == 0 || Cn == 0) return;
    std::vector<double> cost((size_t)R * Cn);
    for (int r = 0; r < R; ++r) {
      const Track& t = tracks[tidx[r]];
      float tb[4];
      if (with_motion) {
        const float m[4] = {(float)t.kf.mean[0], (float)t.kf.mean[1], (float)t.kf.mean[2], (float)t.kf.mean[3]};
        cxcyah_to_xyxy(m, tb);
      } else {
        std::memcpy(tb, t.last_valid, sizeof(tb));
      }
      const float* ko = with_motion ? k_step_observation(t, cfg.vel_delta_t) : nullptr;
      const bool valid = with_motion && !t.vel_placeholder &&
                         (((ko[0] + ko[1]) + ko[2]) + ko[3]) != -4.0f;
      for (int c = 0; c < Cn; ++c) {
        const float* d = dets + (size_t)didx[c] * 8;
        const float dist = cost_entry(tb, d, with_motion, ko, t.vel, valid, cfg.weight_iou_with_det_scores,
                                      cfg.vel_consist_weight);
        cost[(size_t)r * Cn + c] = (double)dist;
      }
    }
    std::vector<int32_t> x(R);
    (void)st_lapjv_extended(cost.data(), R, Cn, 1.0 - (double)cfg.match_iou_thr, x.data(), det_to_row.data());
  }

  // camera-motion compensation of a confirmed track's Kalman state (reference gmc.py:20-45), float64
  static void apply_warp(KState& s, const double* W) {
    const double R[4] = {W[0], W[1], W[3], W[4]}, t[2] = {W[2], W[5]};
    const double det = R[0] * R[3] - R[1] * R[2];
    const double sc = std::sqrt(det > 1e-12 ? det : 1e-12);
    double m[8];
    std::memcpy(m, s.mean, sizeof(m));
    m[0] = R[0] * s.mean[0] + R[1] * s.mean[1] + t[0];
    m[1] = R[2] * s.mean[0] + R[3] * s.mean[1] + t[1];
    m[3] = s.mean[3] * sc;
    m[4] = R[0] * s.mean[4] + R[1] * s.mean[5];
    m[5] = R[2] * s.mean[4] + R[3] * s.mean[5];
    m[7] = s.mean[7] * sc;
    std::memcpy(s.mean, m, sizeof(m));
    double M[64] = {};
    for (int i = 0; i < 8; ++i) M[i * 8 + i] = 1.0;
    M[0] = R[0]; M[1] = R[1]; M[8] = R[2]; M[9] = R[3];
    M[4 * 8 + 4] = R[0]; M[4 * 8 + 5] = R[1]; M[5 * 8 + 4] = R[2]; M[5 * 8 + 5] = R[3];
    M[3 * 8 + 3] = sc; M[7 * 8 + 7] = sc;
    double tmp[64], out[64];     // (M cov) M^T, as numpy's R8x8.dot(cov).dot(R8x8.T)
    for (int i = 0; i < 8; ++i)
      for (int j = 0; j < 8; ++j) {
        double a = 0;
        for (int k = 0; k < 8; ++k) a += M[i * 8 + k] * s.cov[k * 8 + j];
        tmp[i * 8 + j] = a;
      }
    for (int i = 0; i < 8; ++i)
      for (int j = 0; j < 8; ++j) {
        double a = 0;
        for (int k = 0; k < 8; ++k) a += tmp[i * 8 + k] * M[j * 8 + k];
        out[i * 8 + j] = a;
      }
    std::memcpy(s.cov, out, sizeof(out));
  }

  // the reference estimates (and moves its previous CMC image) only in the non-empty branch (:383-445)
  bool nonempty_branch(int frame_id, int n) const { return frame_id != 0 && !tracks.empty() && n > 0; }

  int track(int frame_id, const float* dets, int n, float* out_rows, int64_t* out_ids, int cap, int* out_n,
            const double* warp = nullptr) {
    if (frame_id == 0) reset();
    std::vector<int> order;            // detections of the output, in output order
    std::vector<int64_t> ids;
    if (tracks.empty() || n == 0) {
      for (int i = 0; i < n; ++i)
        if (dets[(size_t)i * 8 + 4] > cfg.init_track_thr) { order.push_back(i); ids.push_back(num_tracks++); }
    } else {
      std::vector<int> cand;           // detections entering association (:409-421)
      for (int i = 0; i < n; ++i)
        if (enters_association(dets + (size_t)i * 8, cfg.obj_score_thr)) cand.push_back(i);
      // 1. KF predict of the confirmed tracks (:431-441)
      std::vector<int> confirmed, tentative;
      for (size_t k = 0; k < tracks.size(); ++k) (tracks[k].tentative ? tentative : confirmed).push_back((int)k);
      for (int k : confirmed) {
        Track& t = tracks[k];
        if (t.last_frame != frame_id - 1) t.kf.mean[7] = 0;
        if (t.tracked) t.saved = t.kf;
        kf_predict(t.kf);
      }
      if (warp)
        for (int k : confirmed) apply_warp(tracks[k].kf, warp);
      std::vector<int> matched_det, matched_trk;    // in the order the reference concatenates them
      std::vector<int32_t> d2r;
      auto apply = [&](const std::vector<int>& tidx, std::vector<int>& pool) {
        std::vector<int> rest;
        for (size_t c = 0; c < pool.size(); ++c) {
          if (d2r[c] > -1) { matched_det.push_back(pool[c]); matched_trk.push_back(tidx[d2r[c]]); }
          else rest.push_back(pool[c]);
        }
        pool.swap(rest);
      };
      // 2. confirmed tracks, 3. tentative tracks (OCM)
      assign(confirmed, cand, dets, true, d2r);
      apply(confirmed, cand);
      assign(tentative, cand, dets, true, d2r);
      apply(tentative, cand);
      // 4. observation-centric recovery on every still-unmatched track (dict order)
      std::vector<char> is_matched(tracks.size(), 0);
      for (int k : matched_trk) is_matched[k] = 1;
      std::vector<int> lost;
      for (size_t k = 0; k < tracks.size(); ++k)
        if (!is_matched[k]) lost.push_back((int)k);
      if (!lost.empty()) {
        assign(lost, cand, dets, false, d2r);
        apply(lost, cand);
        for (int k : matched_trk) is_matched[k] = 1;
      }
      // 5. re-found tracks: smooth the KF over the gap; unmatched tracks: mark lost (:568-581)
      for (size_t i = 0; i < matched_det.size(); ++i) {
        Track& t = tracks[matched_trk[i]];
        if (!t.tracked) online_smooth(t, dets + (size_t)matched_det[i] * 8);
      }
      for (size_t k = 0; k < tracks.size(); ++k)
        if (!is_matched[k]) { tracks[k].tracked = false; push_obs(tracks[k], nullptr, cfg.vel_delta_t); }
      for (size_t i = 0; i < matched_det.size(); ++i) { order.push_back(matched_det[i]); ids.push_back(tracks[matched_trk[i]].id); }
      // 6. new ids for the leftovers (no init threshold on later frames, :588-593)
      for (int di : cand) { order.push_back(di); ids.push_back(num_tracks++); }
    }
    ST_REQUIRE((int)order.size() <= cap, "st_tracker_track: output capacity %d < %zu rows", cap, order.size());
    // BaseTracker.update (:54-91): feed every output row to its track, then pop the invalid ones
    for (size_t i = 0; i < order.size(); ++i) {
      const float* row = dets + (size_t)order[i] * 8;
      const int k = find(ids[i]);
      if (k >= 0) {
        update_track(tracks[k], row, frame_id, cfg.num_tentatives, cfg.vel_delta_t);
      } else {
        tracks.emplace_back(cfg.vel_delta_t);
        init_track(tracks.back(), ids[i], row, frame_id, cfg.vel_delta_t);
      }
      std::memcpy(out_rows + i * 8, row, 8 * sizeof(float));
      out_ids[i] = ids[i];
    }
    for (size_t k = 0; k < tracks.size();) {
      if (is_dropped(&tracks[k], frame_id, cfg.num_frames_retain))
        tracks.erase(tracks.begin() + k);
      else
        ++k;
    }
    *out_n = (int)order.size();
    return ST_OK;
  }
};

extern "C" int st_tracker_create(const StTrackerConfig* cfg, StTracker** out) {
  using namespace st;
  if (!cfg || !out) return set_error(ST_ERR_INVALID, "st_tracker_create: null argument");
  ST_REQUIRE(cfg->struct_size == (int)sizeof(StTrackerConfig), "st_tracker_create: struct_size mismatch");
  ST_REQUIRE(cfg->vel_delta_t >= 0 && cfg->num_tentatives >= 1 && cfg->num_frames_retain >= 1,
             "st_tracker_create: bad vel_delta_t / num_tentatives / num_frames_retain");
  auto t = std::make_unique<StTracker>();
  t->cfg = *cfg;
  *out = t.release();
  return ST_OK;
}

extern "C" int st_tracker_destroy(StTracker* t) {
  delete t;
  return ST_OK;
}

extern "C" int st_tracker_reset(StTracker* t) {
  if (!t) return st::set_error(ST_ERR_INVALID, "st_tracker_reset: null tracker");
  t->reset();
  return ST_OK;
}

extern "C" int st_tracker_track(StTracker* t, int frame_id, const float* dets, int n, float* out_rows,
                                int64_t* out_ids, int cap, int* out_n) {
  using namespace st;
  if (!t || !out_n) return set_error(ST_ERR_INVALID, "st_tracker_track: null argument");
  ST_REQUIRE(n >= 0 && cap >= 0 && (n == 0 || dets) && (cap == 0 || (out_rows && out_ids)),
             "st_tracker_track: bad buffers");
  return t->track(frame_id, dets, n, out_rows, out_ids, cap, out_n);
}

namespace {
// st_tracker_track_records(_cmc): warps == nullptr = no camera-motion compensation
int track_records(StTracker* t, const int* frame_ids, const float* records, int F, int rows_per_frame, int cols,
                  const float* warps, const int* warp_src, int* cmc_prev, float* out_rows, int64_t* out_ids, int cap,
                  int* out_counts, int* stop_at) {
  using namespace st;
  if (!t || !frame_ids || !records || !out_counts)
    return set_error(ST_ERR_INVALID, "st_tracker_track_records: null argument");
  ST_REQUIRE(F >= 0 && rows_per_frame >= 1 && cols >= 12 && cap >= 0 && (cap == 0 || (out_rows && out_ids)),
             "st_tracker_track_records: bad buffers (cols %d: the records must carry the scaled box, mode 2)", cols);
  std::vector<float> dets;
  for (int f = 0; f < F; ++f) {
    const float* rec = records + (size_t)f * rows_per_frame * cols;
    if (rec[2] == 0.0f) {   // batch padding: not a frame
      out_counts[f] = -1;
      continue;
    }
    const int k = (int)rec[0], capacity = (int)rec[1];
    ST_REQUIRE(capacity == rows_per_frame - 1, "st_tracker_track_records: frame %d: record capacity %d != %d rows", f,
               capacity, rows_per_frame - 1);
    if (k > capacity)
      return set_error(ST_ERR_WORKSPACE, "frame %d: %d detections kept but the detection buffer has %d rows",
                       frame_ids[f], k, capacity);
    dets.resize((size_t)k * 8);
    for (int i = 0; i < k; ++i) {
      const float* r = rec + (size_t)(1 + i) * cols;
      float* d = dets.data() + (size_t)i * 8;
      d[0] = r[8]; d[1] = r[9]; d[2] = r[10]; d[3] = r[11];   // the depth-SCALED box (ocsort_disparity.py:82-86)
      d[4] = r[4]; d[5] = r[5]; d[6] = r[6]; d[7] = r[7];
    }
    double wbuf[6];
    const double* warp = nullptr;
    if (warps) {
      if (frame_ids[f] == 0) *cmc_prev = -1;                       // reset_cmc() on the first frame (:385-387)
      if (t->nonempty_branch(frame_ids[f], k)) {
        if (*cmc_prev != -1) {
          if (warp_src[f] != *cmc_prev) {                           // the speculative pair is not (previous CMC image, f)
            *stop_at = f;
            return ST_OK;
          }
          const float* w = warps + (size_t)f * ST_CMC_WARP_FLOATS;
          if (w[0] != 0.f) {
            for (int i = 0; i < 6; ++i) wbuf[i] = (double)w[2 + i];
            warp = wbuf;
          }
        }
        *cmc_prev = frame_ids[f];                                   // estimate_camera_motion stores this image
      }
    }
    float* o = out_rows + (size_t)f * cap * 8;
    int n = 0;
    ST_CHECK(t->track(frame_ids[f], dets.data(), k, o, out_ids + (size_t)f * cap, cap, &n, warp));
    // scale_bbox(track_bboxes, 1 / scales) (ocsort_disparity.py:95-97), in place
    for (int i = 0; i < n; ++i) unscale_box(o + (size_t)i * 8, o + (size_t)i * 8);
    out_counts[f] = n;
  }
  if (stop_at) *stop_at = F;
  return ST_OK;
}
}  // namespace

extern "C" int st_tracker_track_records(StTracker* t, const int* frame_ids, const float* records, int F,
                                        int rows_per_frame, int cols, float* out_rows, int64_t* out_ids, int cap,
                                        int* out_counts) {
  return track_records(t, frame_ids, records, F, rows_per_frame, cols, nullptr, nullptr, nullptr, out_rows, out_ids,
                       cap, out_counts, nullptr);
}

extern "C" int st_tracker_track_records_cmc(StTracker* t, const int* frame_ids, const float* records, int F,
                                            int rows_per_frame, int cols, const float* warps, const int* warp_src,
                                            int* cmc_prev, float* out_rows, int64_t* out_ids, int cap, int* out_counts,
                                            int* stop_at) {
  using namespace st;
  if (!warps || !warp_src || !cmc_prev || !stop_at)
    return set_error(ST_ERR_INVALID, "st_tracker_track_records_cmc: null argument");
  return track_records(t, frame_ids, records, F, rows_per_frame, cols, warps, warp_src, cmc_prev, out_rows, out_ids,
                       cap, out_counts, stop_at);
}

extern "C" int st_tracker_cmc_needed(const StTracker* t, int frame_id, int n) {
  return t && t->nonempty_branch(frame_id, n) ? 1 : 0;
}

extern "C" int st_tracker_track_cmc(StTracker* t, int frame_id, const float* dets, int n, const double* warp,
                                    float* out_rows, int64_t* out_ids, int cap, int* out_n) {
  using namespace st;
  if (!t || !out_n) return set_error(ST_ERR_INVALID, "st_tracker_track_cmc: null argument");
  ST_REQUIRE(n >= 0 && cap >= 0 && (n == 0 || dets) && (cap == 0 || (out_rows && out_ids)),
             "st_tracker_track_cmc: bad buffers");
  return t->track(frame_id, dets, n, out_rows, out_ids, cap, out_n, warp);
}

extern "C" int st_tracker_num_tracks(const StTracker* t) { return t ? (int)t->tracks.size() : 0; }
extern "C" long long st_tracker_next_id(const StTracker* t) { return t ? t->num_tracks : 0; }

extern "C" int st_tracker_get_track(const StTracker* t, int index, int64_t* id, double* mean8, double* cov64,
                                    int* tentative, int* tracked, int* last_frame) {
  using namespace st;
  if (!t || index < 0 || index >= (int)t->tracks.size())
    return set_error(ST_ERR_INVALID, "st_tracker_get_track: bad index %d", index);
  const Track& k = t->tracks[index];
  if (id) *id = k.id;
  if (mean8) std::memcpy(mean8, k.kf.mean, sizeof(k.kf.mean));
  if (cov64) std::memcpy(cov64, k.kf.cov, sizeof(k.kf.cov));
  if (tentative) *tentative = k.tentative;
  if (tracked) *tracked = k.tracked;
  if (last_frame) *last_frame = k.last_frame;
  return ST_OK;
}

extern "C" int st_tracker_get_states(const StTracker* t, StTrackState* out, int cap, int struct_size, int* out_n,
                                     long long* next_id) {
  using namespace st;
  if (!t || !out_n) return set_error(ST_ERR_INVALID, "st_tracker_get_states: null argument");
  ST_REQUIRE(struct_size == (int)sizeof(StTrackState), "st_tracker_get_states: struct_size mismatch");
  const int n = (int)t->tracks.size();
  ST_REQUIRE(cap >= n && (n == 0 || out), "st_tracker_get_states: capacity %d < %d live tracks", cap, n);
  for (int k = 0; k < n; ++k) {
    const Track& s = t->tracks[k];
    ST_REQUIRE(s.win_len <= ST_TRACK_WINDOW,
               "st_tracker_get_states: track %lld keeps a window of %zu observations (vel_delta_t + 1), StTrackState "
               "holds %d", (long long)s.id, (size_t)s.win_len, ST_TRACK_WINDOW);
    StTrackState& o = out[k];
    std::memset(&o, 0, sizeof(o));
    o.struct_size = (int)sizeof(StTrackState);
    o.id = s.id;
    o.tentative = s.tentative; o.tracked = s.tracked; o.last_frame = s.last_frame; o.n_fed = s.n_fed;
    o.n_obs = s.n_obs; o.win_len = s.win_len; o.trailing_none = s.trailing_none;
    o.vel_placeholder = s.vel_placeholder;
    std::memcpy(o.mean, s.kf.mean, sizeof(o.mean));
    std::memcpy(o.cov, s.kf.cov, sizeof(o.cov));
    std::memcpy(o.saved_mean, s.saved.mean, sizeof(o.saved_mean));
    std::memcpy(o.saved_cov, s.saved.cov, sizeof(o.saved_cov));
    for (int w = 0; w < s.win_len; ++w) {
      std::memcpy(o.win[w], s.win[w].data(), sizeof(o.win[w]));
      o.win_valid[w] = s.win_valid[w] != 0;
    }
    std::memcpy(o.last_valid, s.last_valid, sizeof(o.last_valid));
    o.vel[0] = s.vel[0]; o.vel[1] = s.vel[1];
  }
  *out_n = n;
  if (next_id) *next_id = t->num_tracks;
  return ST_OK;
}
