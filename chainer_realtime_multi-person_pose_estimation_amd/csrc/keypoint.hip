// COCO keypoint matching on the device (keypoint_eval.py states it in NumPy: match_np, oks_np, exp_np).
//
// COCOeval's evaluateImg for iouType 'keypoints', every area range and OKS threshold of a batch of
// images in one launch, one workgroup per image, f64 with every operation rounded on its own (the
// tree builds with -ffp-contract=off; the intrinsics say it in the source):
//   phase 1  stable ranks of the detections by descending score (counting; NaN as -inf), the first
//            max_dets kept; their areas; per area range the ground truths' ignore flags and the
//            visiting order "not ignored first"
//   phase 2  the D' x G object keypoint similarities, pairs strided over the threads, kept in LDS
//            (and written out when the caller asked for them)
//   phase 3  the A x T greedy searches, one thread each, the matched set a bit mask in registers
// op_keypoint_match takes detections and ground truths from the host; op_keypoint_match_staged reads
// the detections from the result rows of staged frames where the post-process left them (the kernel
// applies the 18 -> 17 joint map), uploads the ground-truth tables and copies back the match block.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "common.hpp"
#include "ctx.hpp"
#include "oneshot.hpp"

namespace op {
namespace {

constexpr int kKpThreads = 256;
constexpr int kKp = 17;            // COCO keypoints
constexpr int kKpMaxDets = 64;     // ranks fit one wave
constexpr int kKpMaxGt = 128;      // 64 x 128 f64 = 64 KB of OKS in LDS; the matched set two 64-bit masks
constexpr int kKpMaxThrs = 16, kKpMaxAreas = 4;
constexpr int32_t kKpMaxFrames = 1 << 20;
constexpr int64_t kKpMaxRows = 1ll << 24;  // detections, or ground truths, of one call
// LDS: the fixed tables, then max_dets x (most ground truths of a frame) doubles of OKS
constexpr int kLdsOrder = 0;                                       // int32[64]
constexpr int kLdsArea = kLdsOrder + kKpMaxDets * 4;               // double[64]
constexpr int kLdsFlag = kLdsArea + kKpMaxDets * 8;                // uint8[4][128]: bit 0 ignore, bit 1 crowd
constexpr int kLdsVisit = kLdsFlag + kKpMaxAreas * kKpMaxGt;       // uint8[4][128]
constexpr int kLdsOks = kLdsVisit + kKpMaxAreas * kKpMaxGt;        // double[D'][G]
static_assert(kLdsOks % 16 == 0 && kLdsArea % 8 == 0, "LDS carve alignment");
constexpr int kLdsMax = kLdsOks + kKpMaxDets * kKpMaxGt * 8;

struct KpArgs {
  // detections: host form (dt_off != null: frame f's rows [dt_off[f], dt_off[f + 1]) of kpts / scores)
  // or staged form (hdr != null: [frame][4] = status, -, persons, -; frame f's rows at f * frame_rows)
  const double* dt_kpts;
  const double* dt_scores;
  const int32_t* dt_off;
  const int32_t* hdr;
  int32_t frame_rows;  // staged: rows a frame's block holds (the reads stay below it)
  int32_t row;         // doubles per detection row (51, or 54 for pose rows)
  int32_t jmap[kKp];   // joint of the row that is COCO keypoint i
  // ground truths: frame f's are [gt_off[f], gt_off[f + 1])
  const int32_t* gt_off;
  const double* gt_kpts;
  const double* gt_area;
  const double* gt_bbox;
  const uint8_t* gt_ignore;
  const uint8_t* gt_crowd;
  int32_t n_frames, max_dets, n_thrs, n_areas;
  double thrs[kKpMaxThrs], rng[kKpMaxAreas][2], sig[kKp];
  // outputs (M = max_dets, g0 = gt_off[f], G = the frame's ground truths)
  int32_t* status;     // staged: [frame] status, [n_frames + frame] persons found
  double* dt_score;    // [frame][M] the kept detections' scores, in order (null: not wanted)
  int32_t* dt_order;   // [frame][M], -1 past D'
  double* oks;         // [M * g0 + r * G + g] (null: not wanted)
  int32_t* dt_match;   // [frame][A][T][M]
  uint8_t* dt_ignore;  // [frame][A][T][M]
  int32_t* gt_match;   // [A * T * g0 + (a * T + t) * G + g]
  uint8_t* gt_ig;      // [A * g0 + a * G + g]
};

// keypoint_eval.exp_np: e^x for x <= 0; 0 below -708 and for a NaN
__device__ double kp_exp(double x) {
  if (!(x >= -708.0)) return 0.0;
  const double k = rint(__dmul_rn(x, 1.4426950408889634));
  const double r = __dsub_rn(__dsub_rn(x, __dmul_rn(k, 6.93147180369123816490e-01)),
                             __dmul_rn(k, 1.90821492927058770002e-10));
  constexpr double c[14] = {1.0 / 6227020800.0, 1.0 / 479001600.0, 1.0 / 39916800.0, 1.0 / 3628800.0, 1.0 / 362880.0,
                            1.0 / 40320.0,      1.0 / 5040.0,      1.0 / 720.0,      1.0 / 120.0,     1.0 / 24.0,
                            1.0 / 6.0,          1.0 / 2.0,         1.0,              1.0};
  double p = c[0];
#pragma unroll
  for (int i = 1; i < 14; ++i) p = __dadd_rn(__dmul_rn(p, r), c[i]);
  return ldexp(p, (int)k);
}

// np.sum of m <= 17 contiguous doubles (wholebody.pairwise_sum; body.hip's body_sum)
__device__ double kp_sum(const double* q, int m) {
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

// np.maximum(0, v): a NaN stays
__device__ __forceinline__ double kp_pos(double v) { return (v > 0.0 || v != v) ? v : 0.0; }
__device__ __forceinline__ double kp_key(double s) { return s != s ? -INFINITY : s; }

// computeOks of one pair: P the detection's row, Q the ground truth's 17 x 3
__device__ double kp_oks(const KpArgs& a, const double* P, const double* Q, double area, const double* bbox) {
  int k1 = 0;
  for (int i = 0; i < kKp; ++i) k1 += Q[3 * i + 2] > 0.0 ? 1 : 0;
  double x0 = 0.0, x1 = 0.0, y0 = 0.0, y1 = 0.0;
  if (k1 == 0) {
    x0 = __dsub_rn(bbox[0], bbox[2]);
    x1 = __dadd_rn(bbox[0], __dmul_rn(bbox[2], 2.0));
    y0 = __dsub_rn(bbox[1], bbox[3]);
    y1 = __dadd_rn(bbox[1], __dmul_rn(bbox[3], 2.0));
  }
  const double den = __dadd_rn(area, 2.220446049250313e-16);  // np.spacing(1)
  double q[kKp];
  int m = 0;
  for (int i = 0; i < kKp; ++i) {
    if (k1 > 0 && !(Q[3 * i + 2] > 0.0)) continue;
    const double xd = P[3 * a.jmap[i]], yd = P[3 * a.jmap[i] + 1];
    double dx, dy;
    if (k1 > 0) {
      dx = __dsub_rn(xd, Q[3 * i]);
      dy = __dsub_rn(yd, Q[3 * i + 1]);
    } else {
      dx = __dadd_rn(kp_pos(__dsub_rn(x0, xd)), kp_pos(__dsub_rn(xd, x1)));
      dy = __dadd_rn(kp_pos(__dsub_rn(y0, yd)), kp_pos(__dsub_rn(yd, y1)));
    }
    const double s2 = __dmul_rn(a.sig[i], 2.0);
    const double var = __dmul_rn(s2, s2);
    double e = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
    e = __ddiv_rn(__ddiv_rn(__ddiv_rn(e, var), den), 2.0);
    q[m++] = kp_exp(-e);
  }
  return __ddiv_rn(kp_sum(q, m), (double)m);
}

__global__ __launch_bounds__(kKpThreads) void keypoint_match_kernel(KpArgs a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  int32_t* order = (int32_t*)(lds + kLdsOrder);
  double* d_area = (double*)(lds + kLdsArea);
  uint8_t* flag = (uint8_t*)(lds + kLdsFlag);
  uint8_t* visit = (uint8_t*)(lds + kLdsVisit);
  double* oks = (double*)(lds + kLdsOks);
  const int f = blockIdx.x, tid = threadIdx.x;
  const int M = a.max_dets, A = a.n_areas, T = a.n_thrs;
  // the frame's detections and ground truths
  const double* P;
  const double* S;
  int D;
  if (a.hdr) {
    const int status = a.hdr[4 * f];
    const int found = status == OP_OK ? a.hdr[4 * f + 2] : 0;
    if (tid == 0) {
      a.status[f] = status;
      a.status[a.n_frames + f] = found;
    }
    D = found < 0 ? 0 : (found < a.frame_rows ? found : a.frame_rows);
    P = a.dt_kpts + (int64_t)f * a.frame_rows * a.row;
    S = a.dt_scores + (int64_t)f * a.frame_rows;
  } else {
    D = a.dt_off[f + 1] - a.dt_off[f];
    P = a.dt_kpts + (int64_t)a.dt_off[f] * a.row;
    S = a.dt_scores + a.dt_off[f];
  }
  const int64_t g0 = a.gt_off[f];
  const int G = a.gt_off[f + 1] - a.gt_off[f];
  const double* Q = a.gt_kpts + g0 * (kKp * 3);
  const int Dp = D < M ? D : M;

  // ---- phase 1: ranks, detection areas, ignore flags, visiting order ----
  for (int d = tid; d < D; d += kKpThreads) {
    const double key = kp_key(S[d]);
    int rank = 0;
    for (int e = 0; e < D; ++e) {
      const double other = kp_key(S[e]);
      rank += (other > key || (other == key && e < d)) ? 1 : 0;
    }
    if (rank < M) order[rank] = d;
  }
  for (int i = tid; i < A * G; i += kKpThreads) {
    const int ar = i / G, g = i % G;
    const double area = a.gt_area[g0 + g];
    const bool ig = a.gt_ignore[g0 + g] != 0 || area < a.rng[ar][0] || area > a.rng[ar][1];
    flag[ar * kKpMaxGt + g] = (uint8_t)((ig ? 1 : 0) | (a.gt_crowd[g0 + g] ? 2 : 0));
    a.gt_ig[A * g0 + (int64_t)ar * G + g] = ig ? 1 : 0;
  }
  __syncthreads();
  for (int r = tid; r < M; r += kKpThreads) {
    const int64_t at = (int64_t)f * M + r;
    if (r < Dp) {
      const double* p = P + (int64_t)order[r] * a.row;
      // np.max / np.min: a NaN stays
      double lx = p[3 * a.jmap[0]], hx = lx, ly = p[3 * a.jmap[0] + 1], hy = ly;
      for (int i = 1; i < kKp; ++i) {
        const double x = p[3 * a.jmap[i]], y = p[3 * a.jmap[i] + 1];
        if (x < lx || x != x) lx = x;
        if (x > hx || x != x) hx = x;
        if (y < ly || y != y) ly = y;
        if (y > hy || y != y) hy = y;
      }
      d_area[r] = __dmul_rn(__dsub_rn(hx, lx), __dsub_rn(hy, ly));
      a.dt_order[at] = order[r];
      if (a.dt_score) a.dt_score[at] = S[order[r]];
    } else {
      a.dt_order[at] = -1;
      if (a.dt_score) a.dt_score[at] = 0.0;
    }
  }
  for (int i = tid; i < A * G; i += kKpThreads) {
    const int ar = i / G, g = i % G;
    const uint8_t* fl = flag + ar * kKpMaxGt;
    int keep_before = 0, ig_before = 0, keep_all = 0;
    for (int e = 0; e < G; ++e) {
      const int ig = fl[e] & 1;
      keep_all += 1 - ig;
      if (e < g) {
        keep_before += 1 - ig;
        ig_before += ig;
      }
    }
    visit[ar * kKpMaxGt + ((fl[g] & 1) ? keep_all + ig_before : keep_before)] = (uint8_t)g;
  }

  // ---- phase 2: the D' x G similarities ----
  for (int i = tid; i < Dp * G; i += kKpThreads) {
    const int r = i / G, g = i % G;
    const double v = kp_oks(a, P + (int64_t)order[r] * a.row, Q + (int64_t)g * (kKp * 3), a.gt_area[g0 + g],
                            a.gt_bbox + (g0 + g) * 4);
    oks[i] = v;
    if (a.oks) a.oks[(int64_t)M * g0 + i] = v;
  }
  __syncthreads();

  // ---- phase 3: one greedy search per (area range, threshold) ----
  if (tid >= A * T) return;
  const int ar = tid / T, t = tid % T;
  const uint8_t* fl = flag + ar * kKpMaxGt;
  const uint8_t* vis = visit + ar * kKpMaxGt;
  const double lo = a.rng[ar][0], hi = a.rng[ar][1];
  int32_t* dtm = a.dt_match + (((int64_t)f * A + ar) * T + t) * M;
  uint8_t* dti = a.dt_ignore + (((int64_t)f * A + ar) * T + t) * M;
  int32_t* gtm = a.gt_match + (int64_t)A * T * g0 + (int64_t)(ar * T + t) * G;
  for (int g = 0; g < G; ++g) gtm[g] = -1;
  uint64_t matched[2] = {0, 0};
  const double first_bound = fmin(a.thrs[t], 1.0 - 1e-10);
  for (int r = 0; r < M; ++r) {
    if (r >= Dp) {
      dtm[r] = -1;
      dti[r] = 0;
      continue;
    }
    double bound = first_bound;
    int m = -1;
    for (int pos = 0; pos < G; ++pos) {
      const int g = vis[pos];
      if (((matched[g >> 6] >> (g & 63)) & 1) && !(fl[g] & 2)) continue;
      if (m > -1 && !(fl[m] & 1) && (fl[g] & 1)) break;
      const double v = oks[r * G + g];
      if (v < bound) continue;
      bound = v;
      m = g;
    }
    dtm[r] = m;
    if (m > -1) {
      dti[r] = fl[m] & 1;
      gtm[m] = order[r];
      matched[m >> 6] |= 1ull << (m & 63);
    } else {
      dti[r] = (d_area[r] < lo || d_area[r] > hi) ? 1 : 0;
    }
  }
}

LastMs g_keypoint_last;

bool finite_all(const double* v, int64_t n) {
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

// What both entries share of their arguments: the ground-truth tables and the measure's constants.
struct KpTables {
  const int32_t* gt_offsets;
  const double* gt_kpts;
  const double* gt_area;
  const double* gt_bbox;
  const uint8_t* gt_ignore;
  const uint8_t* gt_iscrowd;
  int32_t max_dets, n_thrs;
  const double* thrs;
  int32_t n_areas;
  const double* area_rng;
  const double* sigmas;
};

// Validates them (OP_ERR_INVALID naming the frame) and fills a's constants; *most = the most ground
// truths of one frame
int kp_check(const char* who, int32_t n, const KpTables& t, KpArgs* a, int* most) {
  if (!t.gt_offsets) return invalid(who, "null gt_offsets");
  if (!t.thrs || !t.area_rng || !t.sigmas) return invalid(who, "null thrs, area_rng or sigmas");
  if (t.max_dets < 1 || t.max_dets > kKpMaxDets) return invalid(who, "max_dets must be in 1 .. 64");
  if (t.n_thrs < 1 || t.n_thrs > kKpMaxThrs) return invalid(who, "n_thrs must be in 1 .. 16");
  if (t.n_areas < 1 || t.n_areas > kKpMaxAreas) return invalid(who, "n_areas must be in 1 .. 4");
  if (!finite_all(t.thrs, t.n_thrs)) return invalid(who, "thrs: not finite");
  if (!finite_all(t.area_rng, 2 * (int64_t)t.n_areas)) return invalid(who, "area_rng: not finite");
  if (!finite_all(t.sigmas, kKp)) return invalid(who, "sigmas: not finite");
  for (int i = 0; i < kKp; ++i)
    if (!(t.sigmas[i] > 0.0)) return invalid(who, "sigmas: not positive");
  if (t.gt_offsets[0] != 0) return invalid(who, "gt_offsets: must start at 0");
  *most = 0;
  for (int f = 0; f < n; ++f) {
    const int64_t g = (int64_t)t.gt_offsets[f + 1] - t.gt_offsets[f];
    if (g < 0) return invalid(who, "gt_offsets: frame " + std::to_string(f) + ": decreasing");
    if (g > kKpMaxGt)
      return invalid(who, "gt_offsets: frame " + std::to_string(f) + ": " + std::to_string(g) +
                              " ground truths, at most 128 per frame");
    *most = std::max(*most, (int)g);
  }
  const int64_t G = t.gt_offsets[n];
  if (G > kKpMaxRows) return invalid(who, "more than 16777216 ground truths");
  if (G > 0) {
    if (!t.gt_kpts || !t.gt_area || !t.gt_bbox || !t.gt_ignore || !t.gt_iscrowd) return invalid(who, "null ground-truth table");
    for (int f = 0; f < n; ++f)
      for (int64_t g = t.gt_offsets[f]; g < t.gt_offsets[f + 1]; ++g) {
        if (!std::isfinite(t.gt_area[g]) || t.gt_area[g] < 0.0)
          return invalid(who, "gt_area: frame " + std::to_string(f) + ": not finite or negative");
        if (!finite_all(t.gt_bbox + 4 * g, 4)) return invalid(who, "gt_bbox: frame " + std::to_string(f) + ": not finite");
      }
  }
  a->n_frames = n;
  a->max_dets = t.max_dets;
  a->n_thrs = t.n_thrs;
  a->n_areas = t.n_areas;
  for (int i = 0; i < t.n_thrs; ++i) a->thrs[i] = t.thrs[i];
  for (int i = 0; i < t.n_areas; ++i) {
    a->rng[i][0] = t.area_rng[2 * i];
    a->rng[i][1] = t.area_rng[2 * i + 1];
  }
  for (int i = 0; i < kKp; ++i) a->sig[i] = t.sigmas[i];
  return OP_OK;
}

// One device buffer of 8-byte aligned pieces, packed on the host (the inputs) or laid out for the
// kernel to fill (the outputs)
struct Pieces {
  size_t bytes = 0;
  size_t add(size_t n) {
    const size_t at = bytes;
    bytes += (n + 7) / 8 * 8;
    return at;
  }
};

// The output block of one call, one allocation and one copy back
struct KpBlock {
  Pieces p;
  size_t status_at, score_at, oks_at, order_at, dtm_at, gtm_at, dti_at, gti_at;
  int64_t n, M, A, T, G;
  bool staged, want_oks;
  KpBlock(int64_t n_, const KpTables& t, int64_t G_, bool staged_, bool want_oks_)
      : n(n_), M(t.max_dets), A(t.n_areas), T(t.n_thrs), G(G_), staged(staged_), want_oks(want_oks_) {
    status_at = p.add(staged ? (size_t)n * 2 * 4 : 0);
    score_at = p.add(staged ? (size_t)(n * M) * 8 : 0);
    oks_at = p.add(want_oks ? (size_t)(M * G) * 8 : 0);
    order_at = p.add((size_t)(n * M) * 4);
    dtm_at = p.add((size_t)(n * A * T * M) * 4);
    gtm_at = p.add((size_t)(A * T * G) * 4);
    dti_at = p.add((size_t)(n * A * T * M));
    gti_at = p.add((size_t)(A * G));
  }
  void point(KpArgs* a, char* base) const {
    a->status = staged ? (int32_t*)(base + status_at) : nullptr;
    a->dt_score = staged ? (double*)(base + score_at) : nullptr;
    a->oks = want_oks ? (double*)(base + oks_at) : nullptr;
    a->dt_order = (int32_t*)(base + order_at);
    a->dt_match = (int32_t*)(base + dtm_at);
    a->gt_match = (int32_t*)(base + gtm_at);
    a->dt_ignore = (uint8_t*)(base + dti_at);
    a->gt_ig = (uint8_t*)(base + gti_at);
  }
  void copy_out(const char* host, double* oks, int32_t* dt_order, int32_t* dt_match, uint8_t* dt_ignore,
                int32_t* gt_match, uint8_t* gt_ig) const {
    if (want_oks) memcpy(oks, host + oks_at, (size_t)(M * G) * 8);
    memcpy(dt_order, host + order_at, (size_t)(n * M) * 4);
    memcpy(dt_match, host + dtm_at, (size_t)(n * A * T * M) * 4);
    memcpy(dt_ignore, host + dti_at, (size_t)(n * A * T * M));
    if (G > 0) {
      memcpy(gt_match, host + gtm_at, (size_t)(A * T * G) * 4);
      memcpy(gt_ig, host + gti_at, (size_t)(A * G));
    }
  }
};

// The ground-truth tables in one upload; points a's inputs into it
struct KpGtUpload {
  Pieces p;
  size_t off_at, kp_at, area_at, bbox_at, ig_at, crowd_at;
  std::vector<char> host;
  KpGtUpload(int32_t n, const KpTables& t) {
    const size_t G = (size_t)t.gt_offsets[n];
    off_at = p.add((size_t)(n + 1) * 4);
    kp_at = p.add(G * kKp * 3 * 8);
    area_at = p.add(G * 8);
    bbox_at = p.add(G * 4 * 8);
    ig_at = p.add(G);
    crowd_at = p.add(G);
    host.assign(p.bytes, 0);
    memcpy(host.data() + off_at, t.gt_offsets, (size_t)(n + 1) * 4);
    if (G) {
      memcpy(host.data() + kp_at, t.gt_kpts, G * kKp * 3 * 8);
      memcpy(host.data() + area_at, t.gt_area, G * 8);
      memcpy(host.data() + bbox_at, t.gt_bbox, G * 4 * 8);
      memcpy(host.data() + ig_at, t.gt_ignore, G);
      memcpy(host.data() + crowd_at, t.gt_iscrowd, G);
    }
  }
  void point(KpArgs* a, const char* base) const {
    a->gt_off = (const int32_t*)(base + off_at);
    a->gt_kpts = (const double*)(base + kp_at);
    a->gt_area = (const double*)(base + area_at);
    a->gt_bbox = (const double*)(base + bbox_at);
    a->gt_ignore = (const uint8_t*)(base + ig_at);
    a->gt_crowd = (const uint8_t*)(base + crowd_at);
  }
};

// Queues the kernel over a's frames with LDS for `most` ground truths a frame, and the copy of the
// output block into `host`; ends the job's timing
void kp_run(Job& job, const KpArgs& a, int most, const char* d_out, std::vector<char>& host) {
  if (job.ok()) {
    const size_t lds = (size_t)kLdsOks + (size_t)a.max_dets * most * 8;
    job.check(hipFuncSetAttribute((const void*)keypoint_match_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax),
              "hipFuncSetAttribute");
    if (job.ok()) {
      hipLaunchKernelGGL(keypoint_match_kernel, dim3((unsigned)a.n_frames), dim3(kKpThreads), lds, job.stream(), a);
      job.check(hipGetLastError(), "keypoint_match_kernel");
    }
  }
  job.end();
  job.download(host.data(), d_out, host.size());
}

}  // namespace
}  // namespace op

using namespace op;

extern "C" int op_keypoint_match(int32_t device, int32_t n_frames, const int32_t* dt_offsets, const double* dt_kpts,
                                 const double* dt_scores, const int32_t* gt_offsets, const double* gt_kpts,
                                 const double* gt_area, const double* gt_bbox, const uint8_t* gt_ignore,
                                 const uint8_t* gt_iscrowd, int32_t max_dets, int32_t n_thrs, const double* thrs,
                                 int32_t n_areas, const double* area_rng, const double* sigmas, int32_t* dt_order,
                                 double* oks, int32_t* dt_match, uint8_t* dt_ignore, int32_t* gt_match,
                                 uint8_t* gt_ignore_out) {
  const char* who = "op_keypoint_match";
  if (n_frames < 0 || n_frames > kKpMaxFrames) return invalid(who, "n_frames must be in 0 .. 1048576");
  if (n_frames == 0) return OP_OK;
  if (!dt_offsets) return invalid(who, "null dt_offsets");
  const KpTables t{gt_offsets, gt_kpts, gt_area, gt_bbox, gt_ignore, gt_iscrowd, max_dets, n_thrs, thrs, n_areas, area_rng, sigmas};
  KpArgs a{};
  int most = 0;
  RC(kp_check(who, n_frames, t, &a, &most));
  if (dt_offsets[0] != 0) return invalid(who, "dt_offsets: must start at 0");
  for (int f = 0; f < n_frames; ++f)
    if (dt_offsets[f + 1] < dt_offsets[f]) return invalid(who, "dt_offsets: frame " + std::to_string(f) + ": decreasing");
  const int64_t D = dt_offsets[n_frames], G = gt_offsets[n_frames];
  if (D > kKpMaxRows) return invalid(who, "more than 16777216 detections");
  if (D > 0 && (!dt_kpts || !dt_scores)) return invalid(who, "null dt_kpts or dt_scores");
  if (!dt_order || !dt_match || !dt_ignore) return invalid(who, "null output");
  if (G > 0 && (!gt_match || !gt_ignore_out)) return invalid(who, "null output");
  RC(use_device(who, device));
  const KpBlock blk(n_frames, t, G, false, oks != nullptr);
  const KpGtUpload up(n_frames, t);
  std::vector<char> host(blk.p.bytes);
  Job job(who, nullptr);
  char* d_gt = (char*)job.alloc(up.p.bytes);
  int32_t* d_off = (int32_t*)job.alloc((size_t)(n_frames + 1) * 4);
  double* d_kp = (double*)job.alloc((size_t)D * kKp * 3 * 8);
  double* d_sc = (double*)job.alloc((size_t)D * 8);
  char* d_out = (char*)job.alloc(blk.p.bytes);
  job.begin();
  job.upload(d_gt, up.host.data(), up.p.bytes);
  job.upload(d_off, dt_offsets, (size_t)(n_frames + 1) * 4);
  job.upload(d_kp, dt_kpts, (size_t)D * kKp * 3 * 8);
  job.upload(d_sc, dt_scores, (size_t)D * 8);
  up.point(&a, d_gt);
  a.dt_off = d_off;
  a.dt_kpts = d_kp;
  a.dt_scores = d_sc;
  a.row = kKp * 3;
  for (int i = 0; i < kKp; ++i) a.jmap[i] = i;
  blk.point(&a, d_out);
  kp_run(job, a, most, d_out, host);
  if (job.finish("kernel")) return job.status();
  blk.copy_out(host.data(), oks, dt_order, dt_match, dt_ignore, gt_match, gt_ignore_out);
  g_keypoint_last.done(device, job.ms());
  return OP_OK;
}

extern "C" int op_keypoint_match_staged(op_ctx* c, int32_t first, int32_t n, const int32_t* joint_map,
                                        const int32_t* gt_offsets, const double* gt_kpts, const double* gt_area,
                                        const double* gt_bbox, const uint8_t* gt_ignore, const uint8_t* gt_iscrowd,
                                        int32_t max_dets, int32_t n_thrs, const double* thrs, int32_t n_areas,
                                        const double* area_rng, const double* sigmas, int32_t* frame_status,
                                        int32_t* dt_count, double* dt_scores, int32_t* dt_order, double* oks,
                                        int32_t* dt_match, uint8_t* dt_ignore, int32_t* gt_match,
                                        uint8_t* gt_ignore_out) {
  const char* who = "op_keypoint_match_staged";
  if (!c) return invalid(who, "null context");
  if (n < 1 || n > kKpMaxFrames) return invalid(who, "n must be in 1 .. 1048576");
  if (!joint_map) return invalid(who, "null joint_map");
  for (int i = 0; i < kKp; ++i)
    if (joint_map[i] < 0 || joint_map[i] >= OP_N_JOINTS) return invalid(who, "joint_map names a joint outside 0 .. 17");
  const KpTables t{gt_offsets, gt_kpts, gt_area, gt_bbox, gt_ignore, gt_iscrowd, max_dets, n_thrs, thrs, n_areas, area_rng, sigmas};
  KpArgs a{};
  int most = 0;
  RC(kp_check(who, n, t, &a, &most));
  const int64_t G = gt_offsets[n];
  if (!frame_status || !dt_count || !dt_scores || !dt_order || !dt_match || !dt_ignore) return invalid(who, "null output");
  if (G > 0 && (!gt_match || !gt_ignore_out)) return invalid(who, "null output");
  RC(staged_range(c, who, first, n));
  if (!c->pb.res_hdr || !c->pb.res_poses || !c->pb.res_scores || c->pn < first + n) {
    set_error("op_keypoint_match_staged: no results of the staged frames (run op_run_staged first)");
    return OP_ERR_STATE;
  }
  RC(check_ctx(c, false));
  const KpBlock blk(n, t, G, true, oks != nullptr);
  const KpGtUpload up(n, t);
  std::vector<char> host(blk.p.bytes);
  // ordered on the context stream, behind a queued run; the result rows are read where they lie
  Job job(who, c->stream);
  char* d_gt = (char*)job.alloc(up.p.bytes);
  char* d_out = (char*)job.alloc(blk.p.bytes);
  job.begin();
  job.upload(d_gt, up.host.data(), up.p.bytes);
  up.point(&a, d_gt);
  a.hdr = c->pb.res_hdr + 4 * (size_t)first;
  a.dt_kpts = c->pb.res_poses + (size_t)first * c->pb.maxs * (OP_N_JOINTS * 3);
  a.dt_scores = c->pb.res_scores + (size_t)first * c->pb.maxs;
  a.frame_rows = c->pb.maxs;
  a.row = OP_N_JOINTS * 3;
  for (int i = 0; i < kKp; ++i) a.jmap[i] = joint_map[i];
  blk.point(&a, d_out);
  kp_run(job, a, most, d_out, host);
  if (job.finish("kernel")) return job.status();
  memcpy(frame_status, host.data() + blk.status_at, (size_t)n * 4);
  memcpy(dt_count, host.data() + blk.status_at + (size_t)n * 4, (size_t)n * 4);
  memcpy(dt_scores, host.data() + blk.score_at, (size_t)n * max_dets * 8);
  blk.copy_out(host.data(), oks, dt_order, dt_match, dt_ignore, gt_match, gt_ignore_out);
  g_keypoint_last.done(c->device, job.ms());
  return OP_OK;
}

extern "C" int op_keypoint_last_ms(int32_t device, double* ms) {
  return g_keypoint_last.get("op_keypoint_last_ms", "op_keypoint_match or op_keypoint_match_staged", device, ms);
}
