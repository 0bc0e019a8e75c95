// The post-process C ABI (peaks, connections, grouping, whole frames) and the read-out of its
// results: the batched buffers, and the uncapped one-frame re-run of a frame that overflows them.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "common.hpp"
#include "ctx.hpp"
#include "host_pack.hpp"

namespace op {

// The device Gaussian table (PostBuffers::gauss_w): the CPU-branch taps (scipy's normalised 2r + 1)
// at 0, the GPU-branch 1-D factor (op_set_peak_mode) at kGaussGpuOff, its early-out factor at kGaussGpuGain
std::vector<double> gauss_table(const op_ctx* c) {
  // (a sigma whose radius passes kMaxR -- 2r + 1 > 33 taps -- is refused by check_shape before any
  // launch; its table is cut at the region's end rather than written past it)
  std::vector<double> t(op::kGaussTable, 0.0);
  const size_t nc = std::min<size_t>(c->gauss_host.size(), op::kGaussGpuOff);
  const size_t ng = std::min<size_t>(c->gpu_taps.size(), op::kGaussTable - op::kGaussGpuOff);
  std::copy(c->gauss_host.begin(), c->gauss_host.begin() + nc, t.begin());
  std::copy(c->gpu_taps.begin(), c->gpu_taps.begin() + ng, t.begin() + op::kGaussGpuOff);
  if (ng) t[op::kGaussGpuGain] = op::gpu_branch_gain(c->gpu_taps);
  return t;
}

int ensure_post(op_ctx* c, int n, int mh, int mw) {
  if (c->pn >= n && c->pmh * c->pmw >= mh * mw && c->pb.up) return OP_OK;
  const int nn = std::max(n, c->pn), area = std::max(mh * mw, c->pmh * c->pmw);
  PostBuffers b{};
  b.maxp = c->lim.max_peaks_per_joint;
  b.maxc = (int64_t)b.maxp * b.maxp;
  b.maxs = OP_N_LIMBS * b.maxp;
  if (b.maxs > 2048) b.maxs = 2048;
  struct Part {
    void** p;
    size_t bytes;
  };
  const size_t plane = (size_t)nn * OP_N_JOINTS * area * sizeof(float);
  std::vector<Part> parts = {
      {(void**)&b.up, plane},
      {(void**)&b.peak_xy, (size_t)nn * OP_N_JOINTS * b.maxp * 4},
      {(void**)&b.peak_score, (size_t)nn * OP_N_JOINTS * b.maxp * 4},
      {(void**)&b.peak_cnt, (size_t)nn * OP_N_JOINTS * 4},
      {(void**)&b.stage_key, (size_t)nn * OP_N_JOINTS * b.maxp * 4},
      {(void**)&b.stage_score, (size_t)nn * OP_N_JOINTS * b.maxp * 4},
      {(void**)&b.cand_score, (size_t)nn * OP_N_LIMBS * b.maxc * 8},
      {(void**)&b.cand_idx, (size_t)nn * OP_N_LIMBS * b.maxc * 4},
      {(void**)&b.cand_cnt, (size_t)nn * OP_N_LIMBS * 4},
      {(void**)&b.conn_ab, (size_t)nn * OP_N_LIMBS * b.maxp * 8},
      {(void**)&b.conn_score, (size_t)nn * OP_N_LIMBS * b.maxp * 8},
      {(void**)&b.conn_cnt, (size_t)nn * OP_N_LIMBS * 4},
      {(void**)&b.sub_ids, 16},
      {(void**)&b.sub_sc, 16},
      {(void**)&b.res_poses, (size_t)nn * b.maxs * OP_N_JOINTS * 3 * 8},
      {(void**)&b.res_scores, (size_t)nn * b.maxs * 8},
      {(void**)&b.res_subsets, (size_t)nn * b.maxs * 20 * 8},
      {(void**)&b.res_hdr, (size_t)nn * 4 * 4},
      {(void**)&b.gauss_w, op::kGaussTable * 8},
  };
  static const char* const part_name[] = {"up",       "peak_xy",    "peak_score",
                                          "peak_cnt", "stage_key", "stage_score", "cand_score", "cand_idx",
                                          "cand_cnt", "conn_ab",   "conn_score", "conn_cnt",   "sub_ids",
                                          "sub_sc",   "res_poses", "res_scores", "res_subsets", "res_hdr",
                                          "gauss_w"};
  size_t total = 0;
  for (auto& q : parts) total += (q.bytes + 255) / 256 * 256 + g_guard;
  OP_HIP_CHECK(hipStreamSynchronize(c->stream));
  if (c->post_arena) {
    guard_forget(c->post_arena, c->post_bytes);
    OP_HIP_CHECK(hipFree(c->post_arena));
  }
  c->post_arena = nullptr;
  OP_HIP_CHECK(hipMalloc(&c->post_arena, total));
  c->post_bytes = total;
  OP_HIP_CHECK(hipMemset(c->post_arena, 0, total));
  char* p = (char*)c->post_arena;
  for (size_t i = 0; i < parts.size(); ++i) {
    *parts[i].p = p;
    p += (parts[i].bytes + 255) / 256 * 256;
    guard_add(part_name[i], p, nullptr);
    p += g_guard;
  }
  OP_HIP_CHECK(hipDeviceSynchronize());
  const std::vector<double> gt = gauss_table(c);
  OP_HIP_CHECK(hipMemcpy(b.gauss_w, gt.data(), gt.size() * 8, hipMemcpyHostToDevice));
  c->pb = b;
  c->pn = nn;
  c->pmh = mh;
  c->pmw = area / mh;
  if (c->gexec) {
    hipGraphExecDestroy(c->gexec);
    c->gexec = nullptr;
  }
  return OP_OK;
}

void post_shape(op_ctx* c, PostShape& s, int n, int lh, int lw, int mh, int mw, double img_len, double sx,
                double sy) {
  s.n = n;
  s.lh = lh;
  s.lw = lw;
  s.mh = mh;
  s.mw = mw;
  s.radius = c->gauss_r;
  s.peak_mode = c->peak_mode;
  s.gpu_radius = c->gpu_r;
  s.img_len = img_len;
  s.sx = sx;
  s.sy = sy;
  s.peak_thresh = (float)c->prm.heatmap_peak_thresh;
  s.n_integ = c->prm.n_integ_points;
  s.n_integ_thresh = c->prm.n_integ_points_thresh;
  s.inner_thresh = c->prm.inner_product_thresh;
  s.len_ratio = c->prm.limb_length_ratio;
  s.len_penalty = c->prm.length_penalty_value;
  s.subset_min = c->prm.n_subset_limbs_thresh;
  s.subset_score = c->prm.subset_score_thresh;
  memcpy(s.limbs, c->prm.limbs_point, sizeof(s.limbs));
}

// compute_optimal_size (pose_detector.py:57-73); np.round is half-to-even (nearbyint).
void optimal_size(int h, int w, int img_size, int stride, int* out_w, int* out_h) {
  const double aspect = (double)h / (double)w;
  int iw, ih;
  if (h < w) {
    ih = img_size;
    iw = (int)std::nearbyint((double)img_size / aspect);
    const int sur = iw % stride;
    if (sur) iw += stride - sur;
  } else {
    iw = img_size;
    ih = (int)std::nearbyint((double)img_size * aspect);
    const int sur = ih % stride;
    if (sur) ih += stride - sur;
  }
  *out_w = iw;
  *out_h = ih;
}

// ---- uncapped post-process (the reference has no caps, pose_detector.py:75-250) ----
// A frame whose peaks per joint exceed the batched buffers' cap, or whose subsets overflow the
// LDS grouping, is re-run alone in "big mode": one-frame buffers sized from its own counts (peaks
// per joint, candidates per limb, subsets <= connections + 1), greedy bitsets and subsets in HBM,
// a rank sort for the peak lists.  Only device memory bounds it (OP_ERR_CAPACITY if an allocation
// fails).
static int big_buffers(op_ctx* c, int maxp, int64_t maxc, PostBuffers** out) {
  maxp = std::max(maxp, 1);
  maxc = std::max<int64_t>(maxc, 1);
  if (c->bb_arena && c->bigb.maxp >= maxp && c->bigb.maxc >= maxc) {
    *out = &c->bigb;
    return OP_OK;
  }
  if (c->bb_arena) {
    maxp = std::max(maxp, c->bigb.maxp);
    maxc = std::max(maxc, c->bigb.maxc);
  }
  if ((int64_t)maxp * maxp >= ((int64_t)1 << 31)) {  // candidate pair indices are int32
    set_error("more than 46340 peaks for one joint");
    return OP_ERR_CAPACITY;
  }
  PostBuffers b{};
  b.maxp = maxp;
  b.maxc = maxc;
  b.maxs = OP_N_LIMBS * maxp + 1;  // every new subset consumes a connection (<= maxp per limb)
  const size_t words = ((size_t)maxp + 31) / 32, P = (size_t)maxp, S = (size_t)b.maxs, C = (size_t)maxc;
  struct Part {
    void** p;
    size_t bytes;
  };
  const Part parts[] = {
      {(void**)&b.peak_xy, OP_N_JOINTS * P * 4},   {(void**)&b.peak_score, OP_N_JOINTS * P * 4},
      {(void**)&b.peak_cnt, OP_N_JOINTS * 4},      {(void**)&b.stage_key, OP_N_JOINTS * P * 4},
      {(void**)&b.stage_score, OP_N_JOINTS * P * 4}, {(void**)&b.cand_score, OP_N_LIMBS * C * 8},
      {(void**)&b.cand_idx, OP_N_LIMBS * C * 4},   {(void**)&b.cand_cnt, OP_N_LIMBS * 4},
      {(void**)&b.conn_ab, OP_N_LIMBS * P * 8},    {(void**)&b.conn_score, OP_N_LIMBS * P * 8},
      {(void**)&b.conn_cnt, OP_N_LIMBS * 4},       {(void**)&b.sub_ids, S * OP_N_JOINTS * 4},
      {(void**)&b.sub_sc, S * 2 * 8},              {(void**)&b.res_poses, S * OP_N_JOINTS * 3 * 8},
      {(void**)&b.res_scores, S * 8},              {(void**)&b.res_subsets, S * 20 * 8},
      {(void**)&b.res_hdr, 4 * 4},                 {(void**)&b.gauss_w, op::kGaussTable * 8},
      {(void**)&b.used, OP_N_LIMBS * 2 * words * 4},
  };
  size_t total = 0;
  for (const Part& q : parts) total += (q.bytes + 255) / 256 * 256;
  OP_HIP_CHECK(hipStreamSynchronize(c->stream));
  if (c->bb_arena) OP_HIP_CHECK(hipFree(c->bb_arena));
  c->bb_arena = nullptr;
  c->bigb = PostBuffers{};
  c->big_frame = -1;
  if (hipMalloc(&c->bb_arena, total) != hipSuccess) {
    (void)hipGetLastError();
    c->bb_arena = nullptr;
    set_error("post-process of a frame needs more device memory than is free (" + std::to_string(total >> 20) +
              " MiB for " + std::to_string(maxp) + " peaks per joint)");
    return OP_ERR_CAPACITY;
  }
  char* p = (char*)c->bb_arena;
  for (const Part& q : parts) {
    *q.p = p;
    p += (q.bytes + 255) / 256 * 256;
  }
  const std::vector<double> gt = gauss_table(c);
  OP_HIP_CHECK(hipMemcpy(b.gauss_w, gt.data(), gt.size() * 8, hipMemcpyHostToDevice));
  c->bigb = b;
  *out = &c->bigb;
  return OP_OK;
}

// Run the post-process of `peaks` (frame 0 of B) from the recorded input of frame f.
static int post_one_frame(op_ctx* c, const PostRecord& r, int f, PostBuffers& B) {
  PostShape s1 = r.s;
  s1.n = 1;
  if (r.kind == 1) {
    MapSource src = r.low;
    src.base += (int64_t)f * src.fstride;
    return launch_post_maps(src, s1, B, c->stream);
  }
  const float* m = r.full + (int64_t)f * r.fstride;
  RC(launch_peaks_from_full(m + (size_t)OP_N_PAF * s1.mh * s1.mw, OP_N_JOINTS, s1.mh, s1.mw, s1, B, c->stream,
                            r.fstride));
  RC(launch_connections_full(m, s1.mh, s1.mw, s1, B, c->stream, r.fstride));
  return launch_grouping(s1, B, c->stream);
}

// Re-run frame f of the recorded post-process input r in big mode, sizing the buffers from the
// frame's batched peak counts at d_cnt (18 int32); *out = buffers holding its result.
int rerun_big_rec(op_ctx* c, const PostRecord& r, int f, const int32_t* d_cnt, PostBuffers** out) {
  if (r.kind == 0 || f < 0 || f >= r.s.n) {
    set_error("post-process capacity exceeded and no recorded input to re-run the frame");
    return OP_ERR_CAPACITY;
  }
  OP_HIP_CHECK(hipStreamSynchronize(c->stream));
  int32_t cnt[OP_N_JOINTS];
  OP_HIP_CHECK(hipMemcpy(cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost));
  int maxp = 1;
  for (int j = 0; j < OP_N_JOINTS; ++j) maxp = std::max(maxp, cnt[j]);
  int64_t maxc = std::min<int64_t>((int64_t)maxp * maxp, (int64_t)1 << 20);
  PostBuffers* B = nullptr;
  c->big_frame = -1;
  for (;;) {
    RC(big_buffers(c, maxp, maxc, &B));
    RC(post_one_frame(c, r, f, *B));
    int32_t cc[OP_N_LIMBS];
    OP_HIP_CHECK(hipMemcpyAsync(cc, B->cand_cnt, sizeof(cc), hipMemcpyDeviceToHost, c->stream));
    OP_HIP_CHECK(hipStreamSynchronize(c->stream));
    int64_t need = 0;
    for (int l = 0; l < OP_N_LIMBS; ++l) need = std::max<int64_t>(need, cc[l]);
    if (need <= B->maxc) break;
    maxc = need;  // more candidates than the first guess: grow and run again
  }
  *out = B;
  return OP_OK;
}

// Re-run frame f of the last batched post-process in big mode (cached per frame).
static int rerun_big(op_ctx* c, int f, PostBuffers** out) {
  if (c->big_frame == f && c->bb_arena) {
    *out = &c->bigb;
    return OP_OK;
  }
  if (c->post_rec.kind == 0 || f < 0 || f >= c->post_rec.s.n) {
    set_error("post-process capacity exceeded and no recorded input to re-run the frame");
    return OP_ERR_CAPACITY;
  }
  RC(rerun_big_rec(c, c->post_rec, f, c->pb.peak_cnt + (size_t)f * OP_N_JOINTS, out));
  c->big_frame = f;
  return OP_OK;
}

// The result of a one-frame big-mode buffer set (frame 0 of B) into the caller's arrays.
int read_big(PostBuffers* B, double* poses, double* scores, int cap, op_frame_result* res) {
  int32_t hdr[4];
  OP_HIP_CHECK(hipMemcpy(hdr, B->res_hdr, sizeof(hdr), hipMemcpyDeviceToHost));
  res->status = hdr[0];
  res->n_peaks = hdr[1];
  res->n_persons = hdr[0] == OP_OK ? hdr[2] : 0;
  if (hdr[0] != OP_OK) {
    set_error(hdr[0] == OP_ERR_INDEX ? "list assignment index out of range (grouping_key_points)"
                                     : "post-process capacity exceeded (peaks per joint / subsets)");
    return hdr[0];
  }
  if (hdr[2] > cap) {
    set_error("result capacity too small");
    return OP_ERR_CAPACITY;
  }
  if (hdr[2] > 0) {
    OP_HIP_CHECK(hipMemcpy(poses, B->res_poses, (size_t)hdr[2] * 54 * 8, hipMemcpyDeviceToHost));
    OP_HIP_CHECK(hipMemcpy(scores, B->res_scores, (size_t)hdr[2] * 8, hipMemcpyDeviceToHost));
  }
  return OP_OK;
}

void post_record(op_ctx* c, int kind, const MapSource* low, const float* full, int64_t fstride,
                 const PostShape& s) {
  c->post_rec.kind = kind;
  if (low) c->post_rec.low = *low;
  c->post_rec.full = full;
  c->post_rec.fstride = fstride;
  c->post_rec.s = s;
  c->big_frame = -1;
}

int read_result(op_ctx* c, int frame, double* poses, double* scores, int cap, op_frame_result* res) {
  int32_t hdr[4];
  OP_HIP_CHECK(hipMemcpy(hdr, c->pb.res_hdr + 4 * frame, sizeof(hdr), hipMemcpyDeviceToHost));
  const PostBuffers* B = &c->pb;
  int slot = frame;
  if (hdr[0] == OP_ERR_CAPACITY && c->post_rec.kind) {  // over the batched caps: re-run uncapped
    PostBuffers* big = nullptr;
    RC(rerun_big(c, frame, &big));
    OP_HIP_CHECK(hipMemcpy(hdr, big->res_hdr, sizeof(hdr), hipMemcpyDeviceToHost));
    B = big;
    slot = 0;
  }
  res->status = hdr[0];
  res->n_peaks = hdr[1];
  res->n_persons = hdr[2];
  if (hdr[0] != OP_OK) {
    set_error(hdr[0] == OP_ERR_INDEX ? "list assignment index out of range (grouping_key_points)"
                                     : "post-process capacity exceeded (peaks per joint / subsets)");
    return hdr[0];
  }
  if (hdr[2] > cap) {
    set_error("result capacity too small");
    return OP_ERR_CAPACITY;
  }
  if (hdr[2] > 0) {
    OP_HIP_CHECK(hipMemcpy(poses, B->res_poses + (size_t)slot * B->maxs * 54, (size_t)hdr[2] * 54 * 8,
                           hipMemcpyDeviceToHost));
    OP_HIP_CHECK(hipMemcpy(scores, B->res_scores + (size_t)slot * B->maxs, (size_t)hdr[2] * 8,
                           hipMemcpyDeviceToHost));
  }
  return OP_OK;
}

}  // namespace op

extern "C" {

// Peaks per joint of (N,5) all_peaks rows (reference format: ordered by joint, ids = row index);
// OP_ERR_INVALID if the rows are not in that format.
static int peaks_per_joint(const double* peaks, int64_t n, int32_t* cnt) {
  for (int j = 0; j < OP_N_JOINTS; ++j) cnt[j] = 0;
  int prev = -1;
  for (int64_t i = 0; i < n; ++i) {
    const double* r = peaks + i * 5;
    const int j = (int)r[0];
    if (j < 0 || j >= OP_N_JOINTS || j < prev || (int64_t)r[4] != i || r[1] < 0 || r[2] < 0 || r[1] > 0xffff ||
        r[2] > 0x7fff) {
      set_error("peaks must be all_peaks rows [joint, x, y, score, id] ordered by joint with id = row");
      return OP_ERR_INVALID;
    }
    prev = j;
    cnt[j]++;
  }
  return OP_OK;
}

// The context's batched post buffers when maxp peaks per joint fit them (and !force_big), else the
// one-frame big-mode buffers sized for maxp / maxc (uncapped: only device memory bounds them).
static int pick_buffers(op_ctx* c, int maxp, int64_t maxc, bool force_big, PostBuffers** out) {
  if (!force_big && maxp <= c->pb.maxp && maxc <= c->pb.maxc) {
    *out = &c->pb;
    return OP_OK;
  }
  return big_buffers(c, std::max(maxp, c->pb.maxp), std::max<int64_t>(maxc, 1), out);
}

// Upload all_peaks rows into the per-joint peak arrays of frame 0 of B.
static int upload_peaks(op_ctx* c, PostBuffers& B, const double* peaks, int64_t n) {
  using namespace op;
  const int maxp = B.maxp;
  std::vector<int32_t> xy((size_t)OP_N_JOINTS * maxp, 0), cnt(OP_N_JOINTS, 0);
  std::vector<float> sc((size_t)OP_N_JOINTS * maxp, 0.0f);
  for (int64_t i = 0; i < n; ++i) {
    const double* r = peaks + i * 5;
    const int j = (int)r[0];
    if (cnt[j] >= maxp) {
      set_error("internal: peak buffers smaller than the peaks per joint");
      return OP_ERR_INVALID;
    }
    xy[(size_t)j * maxp + cnt[j]] = (int32_t)r[1] | ((int32_t)r[2] << 16);
    sc[(size_t)j * maxp + cnt[j]] = (float)r[3];
    cnt[j]++;
  }
  OP_HIP_CHECK(hipMemcpyAsync(B.peak_xy, xy.data(), xy.size() * 4, hipMemcpyHostToDevice, c->stream));
  OP_HIP_CHECK(hipMemcpyAsync(B.peak_score, sc.data(), sc.size() * 4, hipMemcpyHostToDevice, c->stream));
  OP_HIP_CHECK(hipMemcpyAsync(B.peak_cnt, cnt.data(), cnt.size() * 4, hipMemcpyHostToDevice, c->stream));
  OP_HIP_CHECK(hipStreamSynchronize(c->stream));
  return OP_OK;
}

int op_compute_peaks(op_ctx* c, const float* heatmaps, int32_t ch, int32_t h, int32_t w, double* peaks, int64_t cap,
                     int64_t* n_peaks) {
  using namespace op;
  RC(check_ctx(c, false));
  if (!heatmaps || !n_peaks || ch != OP_N_JOINTS + 1 || h < 2 || w < 2) {
    set_error("op_compute_peaks: heatmaps must be (19, h, w)");
    return OP_ERR_INVALID;
  }
  RC(ensure_post(c, 1, h, w));
  OP_HIP_CHECK(hipMemcpyAsync(c->pb.up, heatmaps, (size_t)OP_N_JOINTS * h * w * 4, hipMemcpyHostToDevice, c->stream));
  PostShape s;
  post_shape(c, s, 1, h, w, h, w, (double)w, 1.0, 1.0);
  PostBuffers* B = &c->pb;
  std::vector<int32_t> cnt(OP_N_JOINTS);
  for (;;) {
    RC(launch_peaks_from_full(c->pb.up, OP_N_JOINTS, h, w, s, *B, c->stream));
    OP_HIP_CHECK(hipMemcpyAsync(cnt.data(), B->peak_cnt, cnt.size() * 4, hipMemcpyDeviceToHost, c->stream));
    OP_HIP_CHECK(hipStreamSynchronize(c->stream));
    const int most = *std::max_element(cnt.begin(), cnt.end());
    if (most <= B->maxp) break;
    RC(pick_buffers(c, most, 1, true, &B));  // more peaks than the cap: again, uncapped
  }
  const int maxp = B->maxp;
  std::vector<int32_t> xy((size_t)OP_N_JOINTS * maxp);
  std::vector<float> sc((size_t)OP_N_JOINTS * maxp);
  OP_HIP_CHECK(hipMemcpyAsync(xy.data(), B->peak_xy, xy.size() * 4, hipMemcpyDeviceToHost, c->stream));
  OP_HIP_CHECK(hipMemcpyAsync(sc.data(), B->peak_score, sc.size() * 4, hipMemcpyDeviceToHost, c->stream));
  OP_HIP_CHECK(hipStreamSynchronize(c->stream));
  int64_t total = 0;
  for (int j = 0; j < OP_N_JOINTS; ++j) total += cnt[j];
  if (total > cap) {  // the caller's rows are too few: report how many are needed
    *n_peaks = total;
    set_error("peaks capacity too small");
    return OP_ERR_CAPACITY;
  }
  int64_t k = 0;
  for (int j = 0; j < OP_N_JOINTS; ++j) {
    for (int i = 0; i < cnt[j]; ++i) {
      const int32_t v = xy[(size_t)j * maxp + i];
      double* r = peaks + k * 5;
      r[0] = j;
      r[1] = v & 0xffff;
      r[2] = v >> 16;
      r[3] = (double)sc[(size_t)j * maxp + i];
      r[4] = (double)k;
      ++k;
    }
  }
  *n_peaks = k;
  return OP_OK;
}

int op_compute_connections(op_ctx* c, const float* pafs, int32_t h, int32_t w, const double* peaks, int64_t n_peaks,
                           double img_len, double* conn, int64_t cap, int64_t* conn_off) {
  using namespace op;
  RC(check_ctx(c, false));
  if (!pafs || !conn_off || (n_peaks > 0 && !peaks) || h < 1 || w < 1) {
    set_error("op_compute_connections: bad arguments");
    return OP_ERR_INVALID;
  }
  RC(ensure_post(c, 1, h, w));
  int32_t pj[OP_N_JOINTS];
  RC(peaks_per_joint(peaks, n_peaks, pj));
  const int most = *std::max_element(pj, pj + OP_N_JOINTS);
  const size_t pb = (size_t)OP_N_PAF * h * w * 4;
  RC(ensure_scratch(c, pb));
  OP_HIP_CHECK(hipMemcpyAsync(c->d_scratch, pafs, pb, hipMemcpyHostToDevice, c->stream));
  PostShape s;
  post_shape(c, s, 1, h, w, h, w, img_len, 1.0, 1.0);
  PostBuffers* B = nullptr;
  int64_t maxc = std::min<int64_t>((int64_t)most * most, (int64_t)1 << 20);
  RC(pick_buffers(c, most, most <= c->pb.maxp ? 1 : maxc, false, &B));
  std::vector<int32_t> ccnt(OP_N_LIMBS);
  for (;;) {
    RC(upload_peaks(c, *B, peaks, n_peaks));
    RC(launch_connections_full(c->d_scratch, h, w, s, *B, c->stream));
    OP_HIP_CHECK(hipMemcpyAsync(ccnt.data(), B->cand_cnt, ccnt.size() * 4, hipMemcpyDeviceToHost, c->stream));
    OP_HIP_CHECK(hipStreamSynchronize(c->stream));
    const int64_t need = *std::max_element(ccnt.begin(), ccnt.end());
    if (need <= B->maxc) break;
    RC(pick_buffers(c, most, need, true, &B));  // more candidates than the buffers hold: again
  }
  const int maxp = B->maxp;
  std::vector<int32_t> cnt(OP_N_LIMBS), ab((size_t)OP_N_LIMBS * maxp * 2);
  std::vector<double> sc((size_t)OP_N_LIMBS * maxp);
  OP_HIP_CHECK(hipMemcpyAsync(cnt.data(), B->conn_cnt, cnt.size() * 4, hipMemcpyDeviceToHost, c->stream));
  OP_HIP_CHECK(hipMemcpyAsync(ab.data(), B->conn_ab, ab.size() * 4, hipMemcpyDeviceToHost, c->stream));
  OP_HIP_CHECK(hipMemcpyAsync(sc.data(), B->conn_score, sc.size() * 8, hipMemcpyDeviceToHost, c->stream));
  OP_HIP_CHECK(hipStreamSynchronize(c->stream));
  int64_t total = 0;
  for (int l = 0; l < OP_N_LIMBS; ++l) total += cnt[l];
  if (total > cap) {  // the caller's rows are too few: report how many are needed
    conn_off[OP_N_LIMBS] = total;
    set_error("connection capacity too small");
    return OP_ERR_CAPACITY;
  }
  int64_t k = 0;
  for (int l = 0; l < OP_N_LIMBS; ++l) {
    conn_off[l] = k;
    for (int i = 0; i < cnt[l]; ++i) {
      conn[k * 3 + 0] = ab[((size_t)l * maxp + i) * 2];
      conn[k * 3 + 1] = ab[((size_t)l * maxp + i) * 2 + 1];
      conn[k * 3 + 2] = sc[(size_t)l * maxp + i];
      ++k;
    }
  }
  conn_off[OP_N_LIMBS] = k;
  return OP_OK;
}

int op_grouping(op_ctx* c, const double* conn, const int64_t* conn_off, const double* peaks, int64_t n_peaks,
                double* subsets, int64_t cap, int64_t* n_subsets) {
  using namespace op;
  RC(check_ctx(c, false));
  if (!conn_off || !n_subsets || (n_peaks > 0 && !peaks)) {
    set_error("op_grouping: bad arguments");
    return OP_ERR_INVALID;
  }
  // map size is irrelevant for grouping; keep whatever post buffers exist
  RC(ensure_post(c, 1, std::max(c->pmh, 8), std::max(c->pmw, 8)));
  int32_t pj[OP_N_JOINTS];
  RC(peaks_per_joint(peaks, n_peaks, pj));
  int most = *std::max_element(pj, pj + OP_N_JOINTS);
  // peak id ranges per joint (ids are row indices of all_peaks, grouped by joint)
  int64_t jlo[OP_N_JOINTS], jhi[OP_N_JOINTS];
  for (int j = 0; j < OP_N_JOINTS; ++j) {
    jlo[j] = 0;
    jhi[j] = -1;
  }
  for (int64_t i = n_peaks - 1; i >= 0; --i) jlo[(int)peaks[i * 5]] = i;
  for (int64_t i = 0; i < n_peaks; ++i) jhi[(int)peaks[i * 5]] = i;
  for (int l = 0; l < OP_N_LIMBS; ++l) {
    const int64_t k0 = conn_off[l], k1 = conn_off[l + 1];
    if (k1 < k0 || k1 - k0 > 0x7fffffff) {
      set_error("connection offsets must be non-decreasing");
      return OP_ERR_INVALID;
    }
    most = std::max<int64_t>(most, k1 - k0);
    const int ja = c->prm.limbs_point[l][0], jb = c->prm.limbs_point[l][1];
    for (int64_t i = k0; i < k1; ++i) {
      const int64_t ia = (int64_t)conn[i * 3], ib = (int64_t)conn[i * 3 + 1];
      if (ia < jlo[ja] || ia > jhi[ja] || ib < jlo[jb] || ib > jhi[jb]) {
        set_error("connection ids do not belong to the limb's joints");
        return OP_ERR_INVALID;
      }
    }
  }
  PostBuffers* B = nullptr;
  RC(pick_buffers(c, most, 1, false, &B));
  PostShape s;
  post_shape(c, s, 1, 64, 64, 64, 64, 64.0, 1.0, 1.0);  // map size is unused by grouping
  int32_t hdr[4];
  for (;;) {
    RC(upload_peaks(c, *B, peaks, n_peaks));
    const int maxp = B->maxp;
    std::vector<int32_t> cnt(OP_N_LIMBS, 0), ab((size_t)OP_N_LIMBS * maxp * 2, 0);
    std::vector<double> sc((size_t)OP_N_LIMBS * maxp, 0.0);
    for (int l = 0; l < OP_N_LIMBS; ++l) {
      const int64_t k0 = conn_off[l], k1 = conn_off[l + 1];
      cnt[l] = (int)(k1 - k0);
      for (int64_t i = k0; i < k1; ++i) {
        ab[((size_t)l * maxp + (i - k0)) * 2] = (int32_t)conn[i * 3];
        ab[((size_t)l * maxp + (i - k0)) * 2 + 1] = (int32_t)conn[i * 3 + 1];
        sc[(size_t)l * maxp + (i - k0)] = conn[i * 3 + 2];
      }
    }
    OP_HIP_CHECK(hipMemcpyAsync(B->conn_cnt, cnt.data(), cnt.size() * 4, hipMemcpyHostToDevice, c->stream));
    OP_HIP_CHECK(hipMemcpyAsync(B->conn_ab, ab.data(), ab.size() * 4, hipMemcpyHostToDevice, c->stream));
    OP_HIP_CHECK(hipMemcpyAsync(B->conn_score, sc.data(), sc.size() * 8, hipMemcpyHostToDevice, c->stream));
    RC(launch_grouping(s, *B, c->stream));
    OP_HIP_CHECK(hipMemcpyAsync(hdr, B->res_hdr, sizeof(hdr), hipMemcpyDeviceToHost, c->stream));
    OP_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (hdr[0] != OP_ERR_CAPACITY || B != &c->pb) break;
    RC(pick_buffers(c, most, 1, true, &B));  // more subsets than the LDS grouping holds: again, in HBM
  }
  if (hdr[0] == OP_ERR_INDEX) {
    set_error("list assignment index out of range (grouping_key_points)");
    return OP_ERR_INDEX;
  }
  if (hdr[0] != OP_OK) {
    set_error("grouping capacity exceeded");
    return hdr[0];
  }
  if (hdr[2] > cap) {
    *n_subsets = hdr[2];
    set_error("subsets capacity too small");
    return OP_ERR_CAPACITY;
  }
  if (hdr[2] > 0)
    OP_HIP_CHECK(hipMemcpy(subsets, B->res_subsets, (size_t)hdr[2] * 20 * 8, hipMemcpyDeviceToHost));
  *n_subsets = hdr[2];
  return OP_OK;
}

int op_postprocess(op_ctx* c, const float* paf_low, const float* heat_low, int32_t h, int32_t w, int32_t orig_h,
                   int32_t orig_w, double* poses, double* scores, int32_t cap, op_frame_result* res) {
  using namespace op;
  RC(check_ctx(c, false));
  if (!paf_low || !heat_low || !res || h < 2 || w < 2 || orig_h < 1 || orig_w < 1) {
    set_error("op_postprocess: bad arguments");
    return OP_ERR_INVALID;
  }
  std::vector<float> maps((size_t)57 * h * w);
  memcpy(maps.data(), paf_low, (size_t)38 * h * w * 4);
  memcpy(maps.data() + (size_t)38 * h * w, heat_low, (size_t)19 * h * w * 4);
  float* dm = nullptr;
  RC(stage_maps_dev(c, maps.data(), 1, h, w, &dm));
  int map_w, map_h;
  optimal_size(orig_h, orig_w, c->prm.heatmap_size, 8, &map_w, &map_h);
  RC(ensure_post(c, 1, map_h, map_w));
  MapSource src{dm, (int64_t)57 * h * w, 0, 57, 0, 38};
  PostShape s;
  post_shape(c, s, 1, h, w, map_h, map_w, (double)map_w, (double)orig_w / map_w, (double)orig_h / map_h);
  post_record(c, 1, &src, nullptr, 0, s);
  RC(launch_post_maps(src, s, c->pb, c->stream));
  OP_HIP_CHECK(hipStreamSynchronize(c->stream));
  memset(res, 0, sizeof(*res));
  res->map_w = map_w;
  res->map_h = map_h;
  return read_result(c, 0, poses, scores, cap, res);
}

int op_fetch_result(op_ctx* c, int32_t frame, double* poses, double* scores, int32_t cap, op_frame_result* res) {
  using namespace op;
  RC(check_ctx(c, false));
  if (!res || frame < 0 || frame >= c->st_n) {
    set_error("op_fetch_result: bad frame");
    return OP_ERR_INVALID;
  }
  memset(res, 0, sizeof(*res));
  int in_w, in_h, map_w, map_h;
  staged_sizes(c, &in_w, &in_h, &map_w, &map_h);
  res->map_w = map_w;
  res->map_h = map_h;
  res->net_w = in_w;
  res->net_h = in_h;
  return read_result(c, frame, poses, scores, cap, res);
}

int op_fetch_maps(op_ctx* c, int32_t first, int32_t n, float* pafs, float* heatmaps, int32_t* mh, int32_t* mw) {
  using namespace op;
  RC(check_ctx(c, false));
  if (first < 0 || n < 1 || first + n > c->st_n || !mh || !mw) {
    set_error("op_fetch_maps: bad range");
    return OP_ERR_INVALID;
  }
  int in_w, in_h, map_w, map_h;
  staged_sizes(c, &in_w, &in_h, &map_w, &map_h);
  const int h = c->st_precise ? c->st_h : in_h / 8, w = c->st_precise ? c->st_w : in_w / 8;
  *mh = h;
  *mw = w;
  if (!pafs && !heatmaps) return OP_OK;  // size query
  OP_HIP_CHECK(hipStreamSynchronize(c->stream));
  const size_t hw = (size_t)h * w;
  if (c->st_precise) {  // the averaged maps: planar (57, h, w) per frame
    const size_t fpl = (size_t)(OP_N_PAF + OP_N_HEAT) * hw;
    for (int i = 0; i < n; ++i) {
      const float* f = c->d_psum + (size_t)(first + i) * fpl;
      if (pafs) OP_HIP_CHECK(hipMemcpy(pafs + (size_t)i * OP_N_PAF * hw, f, OP_N_PAF * hw * 4, hipMemcpyDeviceToHost));
      if (heatmaps)
        OP_HIP_CHECK(hipMemcpy(heatmaps + (size_t)i * OP_N_HEAT * hw, f + OP_N_PAF * hw, OP_N_HEAT * hw * 4,
                               hipMemcpyDeviceToHost));
    }
    return OP_OK;
  }
  // single scale: the last-stage maps (NHWC) as the network wrote them
  const Act& m = c->split ? c->buf[B_MAP32] : c->buf[B_CAT];
  if (c->gn < first + n || m.h != h || m.w != w) {
    set_error("op_fetch_maps: no network maps of the staged frames (run op_run_staged first)");
    return OP_ERR_STATE;
  }
  const int paf_off = c->split ? 0 : kCatPaf, heat_off = c->split ? 40 : kCatHeat;
  std::vector<float> t(m.frame_floats());
  for (int i = 0; i < n; ++i) {
    OP_HIP_CHECK(hipMemcpy(t.data(), m.p + (size_t)(first + i) * m.frame_floats(), t.size() * 4, hipMemcpyDeviceToHost));
    const int pw = w + 2 * m.pad;
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        const float* px = t.data() + ((size_t)(y + m.pad) * pw + (x + m.pad)) * m.cs;
        if (pafs)
          for (int k = 0; k < OP_N_PAF; ++k) pafs[((size_t)i * OP_N_PAF + k) * hw + (size_t)y * w + x] = px[paf_off + k];
        if (heatmaps)
          for (int k = 0; k < OP_N_HEAT; ++k)
            heatmaps[((size_t)i * OP_N_HEAT + k) * hw + (size_t)y * w + x] = px[heat_off + k];
      }
  }
  return OP_OK;
}

int op_fetch_results(op_ctx* c, int32_t first, int32_t n, double* poses, double* scores, int32_t cap,
                     op_frame_result* res) {
  using namespace op;
  RC(check_ctx(c, false));
  if (!res || !poses || !scores || first < 0 || n < 1 || first + n > c->st_n || cap < 1) {
    set_error("op_fetch_results: bad range");
    return OP_ERR_INVALID;
  }
  std::vector<int32_t> hdr((size_t)n * 4);
  OP_HIP_CHECK(hipMemcpy(hdr.data(), c->pb.res_hdr + 4 * first, hdr.size() * 4, hipMemcpyDeviceToHost));
  int in_w, in_h, map_w, map_h;
  staged_sizes(c, &in_w, &in_h, &map_w, &map_h);
  int maxp = 0;
  std::vector<int> big;
  for (int i = 0; i < n; ++i) {
    op_frame_result& r = res[i];
    memset(&r, 0, sizeof(r));
    r.status = hdr[4 * i];
    r.n_peaks = hdr[4 * i + 1];
    r.n_persons = r.status == OP_OK ? hdr[4 * i + 2] : 0;
    if (r.status == OP_ERR_CAPACITY && c->post_rec.kind) {  // over the batched caps: uncapped re-run
      big.push_back(i);
      r.n_persons = 0;
      r.status = OP_OK;
    }
    r.map_w = map_w;
    r.map_h = map_h;
    r.net_w = in_w;
    r.net_h = in_h;
    maxp = std::max(maxp, r.n_persons);
  }
  if (maxp > cap) {
    set_error("result capacity too small");
    return OP_ERR_CAPACITY;
  }
  if (maxp > 0) {
    // strided device rows -> packed pinned staging (one async 2D copy each), then host rows
    const size_t prow = (size_t)maxp * 54 * 8, srow = (size_t)maxp * 8;
    const size_t need = (size_t)n * (prow + srow);
    if (need > c->host_stage_bytes) {
      if (c->host_stage) OP_HIP_CHECK(hipHostFree(c->host_stage));
      c->host_stage = nullptr;
      OP_HIP_CHECK(hipHostMalloc((void**)&c->host_stage, need, hipHostMallocDefault));
      c->host_stage_bytes = need;
    }
    char* hp = c->host_stage;
    char* hs = c->host_stage + (size_t)n * prow;
    OP_HIP_CHECK(hipMemcpy2DAsync(hp, prow, c->pb.res_poses + (size_t)first * c->pb.maxs * 54,
                                  (size_t)c->pb.maxs * 54 * 8, prow, n, hipMemcpyDeviceToHost, c->stream));
    OP_HIP_CHECK(hipMemcpy2DAsync(hs, srow, c->pb.res_scores + (size_t)first * c->pb.maxs, (size_t)c->pb.maxs * 8,
                                  srow, n, hipMemcpyDeviceToHost, c->stream));
    OP_HIP_CHECK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < n; ++i) {
      const size_t k = (size_t)res[i].n_persons;
      memcpy((char*)poses + (size_t)i * cap * 54 * 8, hp + i * prow, k * 54 * 8);
      memcpy((char*)scores + (size_t)i * cap * 8, hs + i * srow, k * 8);
    }
  }
  for (int i : big) {  // frames over the batched caps, re-run one at a time in big mode
    op_frame_result& r = res[i];
    const int rc = read_result(c, first + i, poses + (size_t)i * cap * 54, scores + (size_t)i * cap, cap, &r);
    if (rc == OP_ERR_HIP || (rc == OP_ERR_CAPACITY && r.n_persons > cap)) return rc;
    if (rc) {
      r.status = rc;
      r.n_persons = 0;
    }
  }
  return OP_OK;
}

}  // extern "C"
