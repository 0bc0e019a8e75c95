// Face / hand boxes from poses on the device (wholebody.py states them in NumPy: body_rois_np).
//
// PoseDetector.get_unit_length, crop_face's box and crop_hands' boxes (pose_detector.py:267-297,
// 354-399) for every person of a batch in one launch, one thread per person, f64 with every operation
// rounded on its own (the tree builds with -ffp-contract=off; the intrinsics say it in the source):
//   len[i]  = sqrt(dx*dx + dy*dy) for all 19 limbs, absent joints at (0, 0) included
//   unit    = mean of len / divisor over the found base limbs, else over every found limb, summed in
//             NumPy's pairwise order (fewer than 8 terms sequentially, else eight accumulators)
//   face    = trunc(nx - u), trunc(ny - 1.2 u), trunc(nx + u), trunc(ny + 0.8 u)
//   hand    = hand + 0.3 (hand - elbow) when the elbow was found, +- 0.95 u, truncated
// The shift of the hand stays in registers: the poses are only read (the reference shifts them in
// place; the staged result rows must stay what op_fetch_results returns).  A box the ROI detector
// would refuse (op_cpm_detect_rois's checks) is reported as state 2, not raised.
// op_body_rois takes the poses from the host; op_body_rois_staged reads the result rows of staged
// frames where the post-process left them and copies back the headers and the tables only.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "common.hpp"
#include "ctx.hpp"
#include "oneshot.hpp"

namespace op {
namespace {

constexpr int kBodyThreads = 64;
constexpr int64_t kBodyMaxRows = 1ll << 24;  // persons (host) or frames * cap (staged) of one call
constexpr int kPose = OP_N_JOINTS * 3;       // doubles per person row
// JointType (entity.py:12-30)
constexpr int kNose = 0, kRElbow = 3, kRHand = 4, kLElbow = 6, kLHand = 7;

struct BodyArgs {
  const double* poses;   // person rows of 54 doubles
  const int32_t* hdr;    // staged: [frame][4] = status, n_peaks, n_persons, -; null: `rows` persons in frame 0
  int64_t frame_stride;  // doubles from one frame's first row to the next's
  int32_t n_frames, cap;
  int32_t rows;          // persons a frame's rows can hold (the reads stay below it)
  int32_t* count;        // [frame] persons found, [n_frames + frame] status
  double* unit;          // [frame][cap]
  int32_t* box;          // [frame][cap][3][4]
  int32_t* state;        // [frame][cap][3]
  int32_t limb[OP_N_LIMBS][2];
};

// pose_detector.py:278-290: the base limbs and their divisors, every limb's divisor
__constant__ int kUnitBase[5] = {14, 3, 0, 13, 9};
__constant__ double kUnitBaseDiv[5] = {0.85, 2.2, 2.2, 0.85, 0.85};
__constant__ double kUnitAllDiv[OP_N_LIMBS] = {2.2, 1.7, 1.7, 2.2, 1.7, 1.7, 0.6, 0.93, 0.65, 0.85,
                                               0.6, 0.93, 0.65, 0.85, 1.0, 0.2, 0.2, 0.25, 0.25};

// np.sum of m <= 19 contiguous doubles (NumPy's pairwise_sum below its block size)
__device__ double body_sum(const double* q, int m) {
  if (m < 8) {
    double s = 0.0;
    for (int i = 0; i < m; ++i) s = __dadd_rn(s, q[i]);
    return s;
  }
  double r[8];
  for (int j = 0; j < 8; ++j) r[j] = q[j];
  int i = 8;
  for (; i < m - (m % 8); i += 8)
    for (int j = 0; j < 8; ++j) r[j] = __dadd_rn(r[j], q[i + j]);
  double s = __dadd_rn(__dadd_rn(__dadd_rn(r[0], r[1]), __dadd_rn(r[2], r[3])),
                       __dadd_rn(__dadd_rn(r[4], r[5]), __dadd_rn(r[6], r[7])));
  for (; i < m; ++i) s = __dadd_rn(s, q[i]);
  return s;
}

// One box: (l, t, r, b) truncated toward zero; state 2 and zeros where op_cpm_detect_rois would
// refuse it (NaN and the infinities fail the range comparisons)
__device__ void body_box(bool present, double l, double t, double r, double b, int32_t* box, int32_t* state) {
  box[0] = box[1] = box[2] = box[3] = 0;
  if (!present) {
    *state = 0;
    return;
  }
  constexpr double kCoord = 1073741824.0;  // 2^30
  const double v[4] = {trunc(l), trunc(t), trunc(r), trunc(b)};
  bool ok = true;
  for (int k = 0; k < 4; ++k) ok = ok && v[k] >= -kCoord && v[k] <= kCoord;
  if (ok) {
    const int64_t bw = (int64_t)v[2] - (int64_t)v[0], bh = (int64_t)v[3] - (int64_t)v[1];
    ok = bw >= 2 && bh >= 2 && bw * bh < (1ll << 31);
  }
  if (!ok) {
    *state = 2;
    return;
  }
  for (int k = 0; k < 4; ++k) box[k] = (int32_t)v[k];
  *state = 1;
}

__global__ __launch_bounds__(kBodyThreads) void body_rois_kernel(BodyArgs a) {
  const int64_t t = (int64_t)blockIdx.x * kBodyThreads + threadIdx.x;
  if (t >= (int64_t)a.n_frames * a.cap) return;
  const int f = (int)(t / a.cap), k = (int)(t % a.cap);
  int found = a.rows, status = OP_OK;
  if (a.hdr) {
    status = a.hdr[4 * f];
    found = status == OP_OK ? a.hdr[4 * f + 2] : 0;
    if (k == 0) {
      a.count[f] = found;
      a.count[a.n_frames + f] = status;
    }
  }
  double* unit = a.unit + t;
  int32_t* box = a.box + t * 12;
  int32_t* state = a.state + t * 3;
  if (k >= found || k >= a.rows) {  // no such person: a zero row
    *unit = 0.0;
    for (int i = 0; i < 12; ++i) box[i] = 0;
    for (int i = 0; i < 3; ++i) state[i] = 0;
    return;
  }
  const double* P = a.poses + (int64_t)f * a.frame_stride + (int64_t)k * kPose;
  double len[OP_N_LIMBS];
  for (int i = 0; i < OP_N_LIMBS; ++i) {
    const double* ja = P + 3 * a.limb[i][0];
    const double* jb = P + 3 * a.limb[i][1];
    const double dx = __dsub_rn(jb[0], ja[0]), dy = __dsub_rn(jb[1], ja[1]);
    len[i] = __dsqrt_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)));
  }
  bool base = false;
  for (int b = 0; b < 5; ++b) base = base || len[kUnitBase[b]] > 0.0;
  double q[OP_N_LIMBS];
  int m = 0;
  if (base) {
    for (int b = 0; b < 5; ++b)
      if (len[kUnitBase[b]] > 0.0) q[m++] = __ddiv_rn(len[kUnitBase[b]], kUnitBaseDiv[b]);
  } else {
    for (int i = 0; i < OP_N_LIMBS; ++i)
      if (len[i] > 0.0) q[m++] = __ddiv_rn(len[i], kUnitAllDiv[i]);
  }
  // no limb found: 0 / 0, written as the one quiet NaN the statement names (np.nan)
  const double u = m ? __ddiv_rn(body_sum(q, m), (double)m) : __longlong_as_double(0x7ff8000000000000ll);
  *unit = u;
  const double nx = P[3 * kNose], ny = P[3 * kNose + 1];
  body_box(P[3 * kNose + 2] > 0.0, __dsub_rn(nx, u), __dsub_rn(ny, __dmul_rn(u, 1.2)), __dadd_rn(nx, u),
           __dadd_rn(ny, __dmul_rn(u, 0.8)), box, state);
  const double s = __dmul_rn(u, 0.95);
  for (int side = 0; side < 2; ++side) {  // left, right
    const double* hand = P + 3 * (side ? kRHand : kLHand);
    const double* elbow = P + 3 * (side ? kRElbow : kLElbow);
    double x = hand[0], y = hand[1];
    if (elbow[2] > 0.0) {
      x = __dadd_rn(x, __dmul_rn(0.3, __dsub_rn(x, elbow[0])));
      y = __dadd_rn(y, __dmul_rn(0.3, __dsub_rn(y, elbow[1])));
    }
    body_box(hand[2] > 0.0, __dsub_rn(x, s), __dsub_rn(y, s), __dadd_rn(x, s), __dadd_rn(y, s), box + 4 * (1 + side),
             state + 1 + side);
  }
}

// params['limbs_point'] as the library holds it (op_default_params), checked before the kernel indexes with it
int body_limbs(const char* who, int32_t (*limb)[2]) {
  op_params prm;
  const int rc = op_default_params(&prm);
  if (rc) return rc;
  for (int i = 0; i < OP_N_LIMBS; ++i)
    for (int e = 0; e < 2; ++e) {
      if (prm.limbs_point[i][e] < 0 || prm.limbs_point[i][e] >= OP_N_JOINTS)
        return invalid(who, "limbs_point names a joint outside 0 .. 17");
      limb[i][e] = prm.limbs_point[i][e];
    }
  return OP_OK;
}

LastMs g_body_last;

// The output block of one call, one allocation and one copy back: [count | status] (staged only),
// units, boxes, states, in this order, the f64 part 8-byte aligned.
struct BodyBlock {
  size_t count_at = 0, unit_at = 0, box_at = 0, state_at = 0, bytes = 0;
  BodyBlock(int64_t frames_hdr, int64_t rows) {
    count_at = 0;
    unit_at = ((size_t)frames_hdr * 2 * 4 + 7) / 8 * 8;
    box_at = unit_at + (size_t)rows * 8;
    state_at = box_at + (size_t)rows * 12 * 4;
    bytes = state_at + (size_t)rows * 3 * 4;
  }
  void point(BodyArgs* a, char* base) const {
    a->count = (int32_t*)(base + count_at);
    a->unit = (double*)(base + unit_at);
    a->box = (int32_t*)(base + box_at);
    a->state = (int32_t*)(base + state_at);
  }
};

// Queues body_rois_kernel over a's n_frames x cap rows, writing blk's block at d_out, and the block's
// copy into `host`; ends the job's timing
void body_run(Job& job, BodyArgs& a, const BodyBlock& blk, char* d_out, std::vector<char>& host) {
  if (job.ok()) {
    const int64_t rows = (int64_t)a.n_frames * a.cap;
    blk.point(&a, d_out);
    hipLaunchKernelGGL(body_rois_kernel, dim3((unsigned)((rows + kBodyThreads - 1) / kBodyThreads)), dim3(kBodyThreads),
                       0, job.stream(), a);
    job.check(hipGetLastError(), "body_rois_kernel");
  }
  job.end();
  job.download(host.data(), d_out, blk.bytes);
}

}  // namespace
}  // namespace op

using namespace op;

extern "C" int op_body_rois(int32_t device, int32_t n_persons, const double* poses, double* unit, int32_t* box,
                            int32_t* state) {
  const char* who = "op_body_rois";
  if (n_persons < 0 || n_persons > kBodyMaxRows) return invalid(who, "n_persons must be in 0 .. 16777216");
  if (n_persons == 0) return OP_OK;
  if (!poses) return invalid(who, "null poses");
  if (!unit || !box || !state) return invalid(who, "null output");
  BodyArgs a{};
  RC(body_limbs(who, a.limb));
  RC(use_device(who, device));
  const BodyBlock blk(0, n_persons);
  const size_t in_bytes = (size_t)n_persons * kPose * 8;
  std::vector<char> host(blk.bytes);
  Job job(who, nullptr);
  a.poses = (const double*)job.alloc(in_bytes);
  char* d_out = (char*)job.alloc(blk.bytes);
  job.begin();
  job.upload((void*)a.poses, poses, in_bytes);
  a.n_frames = 1;
  a.cap = a.rows = n_persons;
  body_run(job, a, blk, d_out, host);
  if (job.finish("kernel")) return job.status();
  memcpy(unit, host.data() + blk.unit_at, (size_t)n_persons * 8);
  memcpy(box, host.data() + blk.box_at, (size_t)n_persons * 12 * 4);
  memcpy(state, host.data() + blk.state_at, (size_t)n_persons * 3 * 4);
  g_body_last.done(device, job.ms());
  return OP_OK;
}

extern "C" int op_body_rois_staged(op_ctx* c, int32_t first, int32_t n, int32_t cap, int32_t* count,
                                   int32_t* frame_status, double* unit, int32_t* box, int32_t* state) {
  const char* who = "op_body_rois_staged";
  if (!c) return invalid(who, "null context");
  if (!count || !frame_status || !unit || !box || !state) return invalid(who, "null output");
  if (n < 1 || cap < 1 || (int64_t)n * cap > kBodyMaxRows) return invalid(who, "n, cap: n >= 1, cap >= 1 and n * cap <= 16777216");
  RC(staged_range(c, who, first, n));
  if (!c->pb.res_hdr || !c->pb.res_poses || c->pn < first + n) {
    set_error("op_body_rois_staged: no results of the staged frames (run op_run_staged first)");
    return OP_ERR_STATE;
  }
  BodyArgs a{};
  RC(body_limbs(who, a.limb));
  RC(check_ctx(c, false));
  const int64_t rows = (int64_t)n * cap;
  const BodyBlock blk(n, rows);
  std::vector<char> host(blk.bytes);
  // ordered on the context stream, behind a queued run; the result rows are read where they lie
  Job job(who, c->stream);
  char* d_out = (char*)job.alloc(blk.bytes);
  job.begin();
  a.poses = c->pb.res_poses + (size_t)first * c->pb.maxs * kPose;
  a.hdr = c->pb.res_hdr + 4 * (size_t)first;
  a.frame_stride = (int64_t)c->pb.maxs * kPose;
  a.n_frames = n;
  a.cap = cap;
  a.rows = c->pb.maxs;
  body_run(job, a, blk, d_out, host);
  if (job.finish("kernel")) return job.status();
  memcpy(count, host.data() + blk.count_at, (size_t)n * 4);
  memcpy(frame_status, host.data() + blk.count_at + (size_t)n * 4, (size_t)n * 4);
  memcpy(unit, host.data() + blk.unit_at, (size_t)rows * 8);
  memcpy(box, host.data() + blk.box_at, (size_t)rows * 12 * 4);
  memcpy(state, host.data() + blk.state_at, (size_t)rows * 3 * 4);
  g_body_last.done(c->device, job.ms());
  int most = 0;
  for (int i = 0; i < n; ++i) most = std::max(most, count[i]);
  if (most > cap) {  // the caller's rows are too few: count says how many are needed
    set_error("op_body_rois_staged: result capacity too small: " + std::to_string(most) + " rows per frame needed");
    return OP_ERR_CAPACITY;
  }
  return OP_OK;
}

extern "C" int op_body_last_ms(int32_t device, double* ms) {
  return g_body_last.get("op_body_last_ms", "op_body_rois or op_body_rois_staged", device, ms);
}
