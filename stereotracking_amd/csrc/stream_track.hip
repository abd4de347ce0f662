// Multi-stream tracking (MultiStreamTracker, stereotracking_amd/multistream.py): the routing kernels of one TICK - one
// frame from each of up to S video streams - between the dense launch plan, the batched GPU association
// (batched_assoc.hip) and the tick's ONE device->host copy.  Nothing here computes anything new: the kernels move rows
// between the layouts the existing stages use, so that neither the host nor a torch indexing op touches a tick.
//
//   dense chunks (frame records, st_pack_records mode 2, one per chunk of `chunk` slots)
//     -> gather_kernel     tracker input dets (S, max_dets, 8) / counts / frame ids BY STREAM + the detection rows of
//                          the tick record
//     -> st_batched_tracker_step (unchanged)
//     -> unscale_kernel    scale_bbox(track box, 1 / scale) BY SLOT, (chunks * chunk, max_dets, 4): st_box_depth's input
//     -> st_box_depth / st_box_depth_method per chunk (unchanged; the disparity lives per chunk)
//     -> record_kernel     the tick record: per stream a header and the pred_track_instances rows
//
// The tick's routing (which slot of which chunk carries which stream) and the chunks' buffer pointers travel in the
// kernel arguments: a tick needs no host->device copy.  One workgroup per stream (or slot); rows across the lanes.
//
// The unscale is reference mmtrack/models/mot/ocsort_disparity.py:95-97 (trackers/utils.py:58-73 scale_bbox) written as
// the single fp32 operations of unscale_box (ocsort_core.h), which the host routine (ocsort_tracker.cpp, track_records)
// calls too; this file is built with -ffp-contract=off like the rest of the library, so no multiply-add is contracted
// and the boxes are equal to the bit.
#include <cstdint>
#include <cstring>

#include "ocsort_core.h"
#include "st_common.h"

namespace st {
namespace ms {

constexpr int kThreads = 256;
constexpr int kRecCols = 13;   // st_pack_records mode 2

struct Route {
  int stream_of_slot[ST_STREAM_MAX_STREAMS];   // -1: batch padding
  int slot_of_stream[ST_STREAM_MAX_STREAMS];   // -1: the stream has no frame in this tick
  int frame_id[ST_STREAM_MAX_STREAMS];         // by stream
};
struct Ptrs { const float* p[ST_STREAM_MAX_STREAMS]; };   // by chunk

struct Layout { size_t ids, hdr, tracks, dets, bytes; };

__host__ __device__ inline Layout layout(int S, int max_dets, int det_rows) {
  Layout l;
  l.ids = 0;
  l.hdr = l.ids + sizeof(long long) * (size_t)S * max_dets;
  l.tracks = l.hdr + sizeof(int) * (size_t)S * ST_STREAM_HDR_INTS;
  l.dets = l.tracks + sizeof(float) * (size_t)S * max_dets * ST_STREAM_ROW_FLOATS;
  l.bytes = l.dets + sizeof(float) * (size_t)S * det_rows * ST_STREAM_DET_FLOATS;
  return l;
}

__global__ __launch_bounds__(kThreads) void gather_kernel(Route route, Ptrs recs, int chunk, int max_dets, int det_rows,
                                                          float* __restrict__ dets, int* __restrict__ counts,
                                                          int* __restrict__ frame_ids, float* __restrict__ rec_dets) {
  const int s = blockIdx.x;
  const int slot = route.slot_of_stream[s];
  if (slot < 0) {
    if (threadIdx.x == 0) { counts[s] = -1; frame_ids[s] = -1; }
    return;
  }
  const float* rec = recs.p[slot / chunk] + (size_t)(slot % chunk) * (det_rows + 1) * kRecCols;
  const int k = (int)rec[0];                     // TRUE number kept: passed on unclipped (the tracker reports status 2)
  if (threadIdx.x == 0) { counts[s] = k; frame_ids[s] = route.frame_id[s]; }
  const int kd = k < det_rows ? k : det_rows;    // rows the frame record holds
  float* d = dets + (size_t)s * max_dets * 8;
  float* o = rec_dets + (size_t)s * det_rows * ST_STREAM_DET_FLOATS;
  for (int i = threadIdx.x; i < kd; i += kThreads) {
    const float* r = rec + (size_t)(1 + i) * kRecCols;
    const float score = r[4], label = r[5];
    if (i < max_dets) {                          // depth-scaled box, score, label, depth, scale (ocsort_disparity.py:82-86)
      float* t = d + (size_t)i * 8;
      t[0] = r[8]; t[1] = r[9]; t[2] = r[10]; t[3] = r[11];
      t[4] = score; t[5] = label; t[6] = r[6]; t[7] = r[7];
    }
    float* q = o + (size_t)i * ST_STREAM_DET_FLOATS;   // pred_det_instances: unscaled box, score, label, prior (:107-108)
    q[0] = r[0]; q[1] = r[1]; q[2] = r[2]; q[3] = r[3];
    q[4] = score; q[5] = label; q[6] = r[12]; q[7] = 0.f;
  }
}

__global__ __launch_bounds__(kThreads) void unscale_kernel(Route route, int max_dets, const float* __restrict__ rows,
                                                           const int* __restrict__ n_tracks, float* __restrict__ boxes,
                                                           int* __restrict__ box_counts) {
  const int slot = blockIdx.x;
  const int s = route.stream_of_slot[slot];
  int n = s >= 0 ? n_tracks[s] : 0;
  n = n < 0 ? 0 : (n > max_dets ? max_dets : n);
  if (threadIdx.x == 0) box_counts[slot] = n;
  if (n == 0) return;
  const float* src = rows + (size_t)s * max_dets * 8;
  float* dst = boxes + (size_t)slot * max_dets * 4;
  // scalar on purpose: vectorised, the four halvings become v_pk_mul_f32 with the 0.5 broadcast by op_sel_hi - the
  // operand form the library must not contain (tests/test_cpu_oracle_and_abi.py fences it)
#pragma clang loop vectorize(disable) interleave(disable)
  for (int i = threadIdx.x; i < n; i += kThreads) {
    oc::unscale_box(src + (size_t)i * 8, dst + (size_t)i * 4);
  }
}

__global__ __launch_bounds__(kThreads) void record_kernel(Route route, Ptrs depth, Ptrs gt_depth, int has_gt, int chunk,
                                                          int max_dets, const float* __restrict__ rows,
                                                          const long long* __restrict__ ids,
                                                          const int* __restrict__ n_tracks,
                                                          const int* __restrict__ status,
                                                          const int* __restrict__ counts,
                                                          const float* __restrict__ boxes, long long* __restrict__ rec_ids,
                                                          int* __restrict__ rec_hdr, float* __restrict__ rec_tracks) {
  const int s = blockIdx.x;
  const int slot = route.slot_of_stream[s];
  int* hdr = rec_hdr + (size_t)s * ST_STREAM_HDR_INTS;
  if (slot < 0) {
    if (threadIdx.x == 0) { hdr[0] = -1; hdr[1] = 0; hdr[2] = 0; hdr[3] = -1; }
    return;
  }
  int n = n_tracks[s];
  n = n < 0 ? 0 : (n > max_dets ? max_dets : n);
  if (threadIdx.x == 0) { hdr[0] = n; hdr[1] = counts[s]; hdr[2] = status[s]; hdr[3] = route.frame_id[s]; }
  const size_t in_chunk = (size_t)(slot % chunk) * max_dets;
  const float* dp = depth.p[slot / chunk] + in_chunk;
  const float* gp = has_gt ? gt_depth.p[slot / chunk] + in_chunk : dp;   // no gt depth map: gt_depth = depth (:104)
  const float* src = rows + (size_t)s * max_dets * 8;
  const float* bx = boxes + (size_t)slot * max_dets * 4;
  float* dst = rec_tracks + (size_t)s * max_dets * ST_STREAM_ROW_FLOATS;
  for (int i = threadIdx.x; i < n; i += kThreads) {
    const float* r = src + (size_t)i * 8;
    const float* b = bx + (size_t)i * 4;
    float* o = dst + (size_t)i * ST_STREAM_ROW_FLOATS;
    o[0] = b[0]; o[1] = b[1]; o[2] = b[2]; o[3] = b[3];
    o[4] = r[4]; o[5] = r[5]; o[6] = r[7]; o[7] = dp[i]; o[8] = gp[i]; o[9] = 0.f;
    rec_ids[(size_t)s * max_dets + i] = ids[(size_t)s * max_dets + i];   // int64, carried as it is
  }
}

// Validate a tick and build the two routing tables from its slot -> stream list.
int make_route(const StStreamTick* t, Route* r, const char* who) {
  if (!t) return set_error(ST_ERR_INVALID, "%s: null tick", who);
  ST_REQUIRE(t->struct_size == (int)sizeof(StStreamTick), "%s: struct_size mismatch", who);
  ST_REQUIRE(t->streams > 0 && t->streams <= ST_STREAM_MAX_STREAMS, "%s: streams must be in [1, %d]", who,
             ST_STREAM_MAX_STREAMS);
  ST_REQUIRE(t->chunk > 0 && t->num_chunks > 0 && (long long)t->chunk * t->num_chunks <= ST_STREAM_MAX_STREAMS,
             "%s: chunk * num_chunks must be in [1, %d]", who, ST_STREAM_MAX_STREAMS);
  ST_REQUIRE(t->max_dets > 0 && t->det_rows > 0, "%s: bad capacities", who);
  ST_REQUIRE(t->stream_of_slot && t->frame_ids, "%s: null routing table", who);
  for (int s = 0; s < ST_STREAM_MAX_STREAMS; ++s) { r->slot_of_stream[s] = -1; r->stream_of_slot[s] = -1; r->frame_id[s] = -1; }
  const int slots = t->chunk * t->num_chunks;
  for (int i = 0; i < slots; ++i) {
    const int s = t->stream_of_slot[i];
    if (s < 0) continue;
    ST_REQUIRE(s < t->streams, "%s: slot %d names stream %d of %d", who, i, s, t->streams);
    ST_REQUIRE(r->slot_of_stream[s] < 0, "%s: stream %d appears twice in one tick", who, s);
    r->slot_of_stream[s] = i;
    r->stream_of_slot[i] = s;
    r->frame_id[s] = t->frame_ids[s];
  }
  return ST_OK;
}

int make_ptrs(const float* const* host, int n, Ptrs* p, const char* who) {
  std::memset(p, 0, sizeof(Ptrs));
  for (int c = 0; c < n; ++c) {
    ST_REQUIRE(host[c], "%s: null chunk pointer %d", who, c);
    p->p[c] = host[c];
  }
  return ST_OK;
}

}  // namespace ms
}  // namespace st

extern "C" size_t st_stream_record_bytes(int streams, int max_dets, int det_rows) {
  if (streams <= 0 || max_dets <= 0 || det_rows <= 0) return 0;
  return st::ms::layout(streams, max_dets, det_rows).bytes;
}

extern "C" int st_stream_gather(const StStreamTick* tick, const float* const* chunk_records, float* dets_dev,
                                int32_t* counts_dev, int32_t* frame_ids_dev, void* record_dev, st_stream_t stream) {
  using namespace st;
  ms::Route route;
  ms::Ptrs recs;
  ST_CHECK(ms::make_route(tick, &route, "st_stream_gather"));
  ST_REQUIRE(chunk_records && dets_dev && counts_dev && frame_ids_dev && record_dev, "st_stream_gather: null pointer");
  ST_CHECK(ms::make_ptrs(chunk_records, tick->num_chunks, &recs, "st_stream_gather"));
  const ms::Layout l = ms::layout(tick->streams, tick->max_dets, tick->det_rows);
  hipLaunchKernelGGL(ms::gather_kernel, dim3(tick->streams), dim3(ms::kThreads), 0, static_cast<hipStream_t>(stream),
                     route, recs, tick->chunk, tick->max_dets, tick->det_rows, dets_dev, counts_dev, frame_ids_dev,
                     reinterpret_cast<float*>(static_cast<char*>(record_dev) + l.dets));
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

extern "C" int st_stream_unscale(const StStreamTick* tick, const float* rows_dev, const int32_t* out_counts_dev,
                                 float* boxes_dev, int32_t* box_counts_dev, st_stream_t stream) {
  using namespace st;
  ms::Route route;
  ST_CHECK(ms::make_route(tick, &route, "st_stream_unscale"));
  ST_REQUIRE(rows_dev && out_counts_dev && boxes_dev && box_counts_dev, "st_stream_unscale: null pointer");
  hipLaunchKernelGGL(ms::unscale_kernel, dim3(tick->chunk * tick->num_chunks), dim3(ms::kThreads), 0,
                     static_cast<hipStream_t>(stream), route, tick->max_dets, rows_dev, out_counts_dev, boxes_dev,
                     box_counts_dev);
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}

extern "C" int st_stream_record(const StStreamTick* tick, const float* rows_dev, const int64_t* ids_dev,
                                const int32_t* out_counts_dev, const int32_t* status_dev, const int32_t* counts_dev,
                                const float* boxes_dev, const float* const* chunk_depth,
                                const float* const* chunk_gt_depth, void* record_dev, st_stream_t stream) {
  using namespace st;
  ms::Route route;
  ms::Ptrs depth, gt;
  ST_CHECK(ms::make_route(tick, &route, "st_stream_record"));
  ST_REQUIRE(rows_dev && ids_dev && out_counts_dev && status_dev && counts_dev && boxes_dev && chunk_depth && record_dev,
             "st_stream_record: null pointer");
  ST_CHECK(ms::make_ptrs(chunk_depth, tick->num_chunks, &depth, "st_stream_record"));
  std::memset(&gt, 0, sizeof(gt));
  if (chunk_gt_depth) ST_CHECK(ms::make_ptrs(chunk_gt_depth, tick->num_chunks, &gt, "st_stream_record"));
  const ms::Layout l = ms::layout(tick->streams, tick->max_dets, tick->det_rows);
  char* rec = static_cast<char*>(record_dev);
  hipLaunchKernelGGL(ms::record_kernel, dim3(tick->streams), dim3(ms::kThreads), 0, static_cast<hipStream_t>(stream),
                     route, depth, gt, chunk_gt_depth ? 1 : 0, tick->chunk, tick->max_dets, rows_dev,
                     reinterpret_cast<const long long*>(ids_dev), out_counts_dev, status_dev, counts_dev, boxes_dev,
                     reinterpret_cast<long long*>(rec + l.ids), reinterpret_cast<int*>(rec + l.hdr),
                     reinterpret_cast<float*>(rec + l.tracks));
  ST_CHECK_HIP(hipGetLastError());
  return ST_OK;
}
