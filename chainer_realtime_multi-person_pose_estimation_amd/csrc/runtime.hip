// Context lifetime, settings, profiling read-out and debugging aids of the MI355X OpenPose path's
// C ABI (include/openpose_hip.h).  The context itself is ctx.hpp; the weights are weights.hip, the
// forward plan forward.hip, the post-process entry points post_api.hip, frame staging and graph
// capture staged.hip, the result records gather.hip and the multi-scale path precise.hip.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "common.hpp"
#include "ctx.hpp"
#include "host_pack.hpp"

namespace op {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }

// ---- debugging aid: guard bands (OP_GUARD=<bytes>) ----
// Every device buffer gets a band of 0xA5 bytes after it; guard_check() (after each debug-synced
// launch and at every synchronising entry point) reports the first band a kernel wrote into.
size_t g_guard = 0;
struct GuardBand {
  const char* name;
  const char* p;
};
static std::vector<GuardBand> g_bands;
static std::mutex g_band_mu;

void guard_add(const char* name, void* p, hipStream_t st) {
  if (!g_guard) return;
  hipMemsetAsync(p, 0xA5, g_guard, st);
  std::lock_guard<std::mutex> lk(g_band_mu);
  g_bands.push_back({name, (const char*)p});
}

void guard_forget(const void* base, size_t bytes) {
  if (!g_guard || !base) return;
  std::lock_guard<std::mutex> lk(g_band_mu);
  const char* b = (const char*)base;
  std::vector<GuardBand> keep;
  for (auto& g : g_bands)
    if (!(g.p >= b && g.p < b + bytes)) keep.push_back(g);
  g_bands.swap(keep);
}

int guard_check(const char* where) {
  if (!g_guard) return OP_OK;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipDeviceSynchronize() != hipSuccess) return OP_OK;  // the caller reports the fault itself
  std::lock_guard<std::mutex> lk(g_band_mu);
  std::vector<unsigned char> h(g_guard);
  for (auto& g : g_bands) {
    if (hipMemcpy(h.data(), g.p, g_guard, hipMemcpyDeviceToHost) != hipSuccess) {
      (void)hipGetLastError();  // a band of a buffer freed without guard_forget: not a kernel fault,
      continue;                 // and the sticky error must not surface at the next launch check
    }
    for (size_t i = 0; i < g_guard; ++i)
      if (h[i] != 0xA5) {
        char msg[256];
        snprintf(msg, sizeof(msg), "guard band after buffer '%s' overwritten at +%zu (byte 0x%02x), seen after %s",
                 g.name, i, h[i], where);
        fprintf(stderr, "[openpose_hip] %s\n", msg);
        set_error(msg);
        (void)cs;
        return OP_ERR_STATE;
      }
  }
  return OP_OK;
}

bool g_debug_sync = false;
int debug_after_launch(const char* name, hipStream_t st) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) return OP_OK;
  const hipError_t e1 = hipGetLastError();
  const hipError_t e2 = hipStreamSynchronize(st);
  if (e1 != hipSuccess || e2 != hipSuccess) {
    set_error(std::string("after kernel ") + name + ": " + hipGetErrorString(e1 != hipSuccess ? e1 : e2));
    fprintf(stderr, "[openpose_hip] fault after kernel %s: %s\n", name, hipGetErrorString(e1 != hipSuccess ? e1 : e2));
    return OP_ERR_HIP;
  }
  return guard_check(name);
}

// (Re)allocate a growable device buffer of `bytes` (+ debug guard band after it).
int grow_buffer(op_ctx* c, void** p, size_t* cap, size_t bytes, const char* name) {
  if (bytes <= *cap) return OP_OK;
  OP_HIP_CHECK(hipStreamSynchronize(c->stream));
  if (c->main_stream) OP_HIP_CHECK(hipStreamSynchronize(c->main_stream));
  if (c->side_stream) OP_HIP_CHECK(hipStreamSynchronize(c->side_stream));
  if (*p) {
    guard_forget(*p, *cap + g_guard);
    OP_HIP_CHECK(hipFree(*p));
  }
  *p = nullptr;
  *cap = 0;  // a failed allocation below leaves no buffer, and says so
  OP_HIP_CHECK(hipMalloc(p, bytes + g_guard));
  *cap = bytes;
  guard_add(name, (char*)*p + bytes, nullptr);
  OP_HIP_CHECK(hipDeviceSynchronize());
  return OP_OK;
}

int ensure_scratch(op_ctx* c, size_t bytes) {
  return grow_buffer(c, (void**)&c->d_scratch, &c->scratch_bytes, bytes, "scratch");
}

hipEvent_t pool_event(op_ctx* c) {
  if (c->ev_used == c->ev_pool.size()) {
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    c->ev_pool.push_back(e);
  }
  return c->ev_pool[c->ev_used++];
}

// Default split-path conv kernel family of new contexts (op_set_conv_algo; OP_HALO_MODE env).
static int g_halo_mode = 4;

int check_ctx(op_ctx* c, bool need_weights) {
  if (!c) {
    set_error("null context");
    return OP_ERR_INVALID;
  }
  if (need_weights && !c->have_weights) {
    set_error("weights not set (op_set_weights)");
    return OP_ERR_STATE;
  }
  OP_HIP_CHECK(hipSetDevice(c->device));
  return OP_OK;
}

static void free_pc(PackedConv& p) {
  if (p.w) hipFree(p.w);
  if (p.b) hipFree(p.b);
  if (p.ws) hipFree(p.ws);
  p.w = p.b = nullptr;
  p.ws = nullptr;
}

void free_weights(op_ctx* c) {
  if (c->w11) hipFree(c->w11);
  c->w11 = nullptr;
  for (auto& p : c->bb) free_pc(p);
  free_pc(c->s1_first);
  for (auto& a : c->s1_g)
    for (auto& p : a) free_pc(p);
  for (auto& p : c->s1_last) free_pc(p);
  for (auto& p : c->st_first) free_pc(p);
  for (auto& a : c->st_g)
    for (auto& b : a)
      for (auto& p : b) free_pc(p);
  for (auto& a : c->st_last)
    for (auto& p : a) free_pc(p);
  c->have_weights = false;
}

}  // namespace op

// =============================== C ABI ===============================
extern "C" {

const char* op_last_error(void) { return op::g_err.c_str(); }

int op_default_params(op_params* p) {
  if (!p) return OP_ERR_INVALID;
  memset(p, 0, sizeof(*p));
  p->inference_img_size = 368;
  p->heatmap_size = 320;
  p->gaussian_sigma = 2.5;
  p->n_integ_points = 10;
  p->n_integ_points_thresh = 8;
  p->heatmap_peak_thresh = 0.05;
  p->inner_product_thresh = 0.05;
  p->limb_length_ratio = 1.0;
  p->length_penalty_value = 1.0;
  p->n_subset_limbs_thresh = 3;
  p->subset_score_thresh = 0.2;
  static const int32_t limbs[OP_N_LIMBS][2] = {{1, 8},  {8, 9},   {9, 10}, {1, 11},  {11, 12}, {12, 13}, {1, 2},
                                               {2, 3},  {3, 4},   {2, 16}, {1, 5},   {5, 6},   {6, 7},   {5, 17},
                                               {1, 0},  {0, 14},  {0, 15}, {14, 16}, {15, 17}};
  memcpy(p->limbs_point, limbs, sizeof(limbs));
  p->downscale = 8;
  p->n_scales = 4;
  p->inference_scales[0] = 0.5;
  p->inference_scales[1] = 1.0;
  p->inference_scales[2] = 1.5;
  p->inference_scales[3] = 2.0;
  return OP_OK;
}

int op_default_limits(op_limits* l) {
  if (!l) return OP_ERR_INVALID;
  l->max_batch = 1;
  l->max_net_h = 368;
  l->max_net_w = 656;
  l->max_map_h = 320;
  l->max_map_w = 576;
  l->max_peaks_per_joint = 512;
  l->max_frame_h = 720;
  l->max_frame_w = 1280;
  return OP_OK;
}

int op_create(const op_params* params, const op_limits* limits, int device, op_ctx** out) {
  if (!out) return OP_ERR_INVALID;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    op::set_error("no HIP device available (this path runs on MI355X only)");
    return OP_ERR_HIP;
  }
  if (device < 0 || device >= ndev) {
    op::set_error("device ordinal out of range");
    return OP_ERR_INVALID;
  }
  op_ctx* c = new op_ctx();
  c->device = device;
  if (params) c->prm = *params;
  else op_default_params(&c->prm);
  op_default_limits(&c->lim);
  if (limits) {
    if (limits->max_batch > 0) c->lim.max_batch = limits->max_batch;
    if (limits->max_net_h > 0) c->lim.max_net_h = limits->max_net_h;
    if (limits->max_net_w > 0) c->lim.max_net_w = limits->max_net_w;
    if (limits->max_map_h > 0) c->lim.max_map_h = limits->max_map_h;
    if (limits->max_map_w > 0) c->lim.max_map_w = limits->max_map_w;
    if (limits->max_peaks_per_joint > 0) c->lim.max_peaks_per_joint = limits->max_peaks_per_joint;
    if (limits->max_frame_h > 0) c->lim.max_frame_h = limits->max_frame_h;
    if (limits->max_frame_w > 0) c->lim.max_frame_w = limits->max_frame_w;
  }
  if (c->lim.max_peaks_per_joint > 2048 || c->prm.n_integ_points > 16 || c->prm.n_integ_points < 2 ||
      c->prm.n_scales < 0 || c->prm.n_scales > OP_MAX_SCALES || c->prm.downscale != 8) {
    op::set_error("parameters outside kernel support (max_peaks_per_joint <= 2048, 2 <= n_integ_points <= 16, "
                  "n_scales <= OP_MAX_SCALES, downscale == 8)");
    delete c;
    return OP_ERR_INVALID;
  }
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    op::set_error("hipStreamCreate failed");
    delete c;
    return OP_ERR_HIP;
  }
  if (op::conv_big_device_init(device) != OP_OK) {
    hipStreamDestroy(c->stream);
    delete c;
    return OP_ERR_HIP;
  }
  for (int i = 0; i < 4; ++i) hipEventCreate(&c->ev[i]);
  if (const char* e = getenv("OP_HALO_MODE")) {
    const int m = atoi(e);
    if (m == 0 || m == 3 || m == 4 || m == 5) op::g_halo_mode = m;
  }
  c->conv_algo = op::g_halo_mode;
  c->stage_planar = !(getenv("OP_STAGE_PLANAR") && atoi(getenv("OP_STAGE_PLANAR")) == 0);
  if (const char* e = getenv("OP_DEBUG_SYNC")) op::g_debug_sync = e[0] == '1';
  if (const char* e = getenv("OP_GUARD")) op::g_guard = ((size_t)atol(e) + 255) / 256 * 256;
  // scipy _gaussian_kernel1d(sigma, 0, int(4*sigma + 0.5)) taps (restated; pinned by the tests)
  c->gauss_r = op::gaussian_taps(c->prm.gaussian_sigma, c->gauss_host);
  *out = c;
  return OP_OK;
}

int op_destroy(op_ctx* c) {
  if (!c) return OP_OK;
  hipSetDevice(c->device);
  if (c->stream) hipStreamSynchronize(c->stream);
  if (c->side_stream) hipStreamSynchronize(c->side_stream);
  if (c->copy_stream) hipStreamSynchronize(c->copy_stream);
  if (c->gexec) hipGraphExecDestroy(c->gexec);
  if (c->graph) hipGraphDestroy(c->graph);
  free_weights(c);
  for (auto& e : c->arenas) {
    guard_forget(e.p, e.bytes);
    hipFree(e.p);
  }
  c->arenas.clear();
  c->arena = nullptr;
  guard_forget(c->post_arena, c->post_bytes);
  guard_forget(c->d_frames, c->frames_bytes + g_guard);
  guard_forget(c->d_maps, c->maps_bytes + g_guard);
  guard_forget(c->d_scratch, c->scratch_bytes + g_guard);
  guard_forget(c->d_fmaps, c->fmaps_bytes + g_guard);
  if (c->post_arena) hipFree(c->post_arena);
  if (c->d_frames) hipFree(c->d_frames);
  if (c->d_maps) hipFree(c->d_maps);
  if (c->d_fmaps) hipFree(c->d_fmaps);
  if (c->d_scratch) hipFree(c->d_scratch);
  guard_forget(c->d_pmid, c->pmid_bytes + g_guard);
  guard_forget(c->d_psum, c->psum_bytes + g_guard);
  if (c->d_pmid) hipFree(c->d_pmid);
  if (c->d_psum) hipFree(c->d_psum);
  if (c->host_stage) hipHostFree(c->host_stage);
  if (c->up_pinned) hipHostFree(c->up_pinned);
  if (c->jpeg_pinned) hipHostFree(c->jpeg_pinned);
  guard_forget(c->d_jpeg, c->jpeg_bytes + g_guard);
  if (c->d_jpeg) hipFree(c->d_jpeg);
  for (auto& k : c->keep) {
    if (k.h_rows) hipHostFree(k.h_rows);
    if (k.maps) hipFree(k.maps);
    if (k.res) hipFree(k.res);
    if (k.cnt) hipFree(k.cnt);
    if (k.d_hdr) hipFree(k.d_hdr);
    if (k.h_hdr) hipHostFree(k.h_hdr);
  }
  if (c->bb_arena) hipFree(c->bb_arena);
  for (auto& e : c->ev)
    if (e) hipEventDestroy(e);
  for (auto& e : c->ev_pool) hipEventDestroy(e);
  if (c->copy_stream) {
    (void)hipStreamSynchronize(c->copy_stream);
    (void)hipStreamDestroy(c->copy_stream);
  }
  if (c->side_stream) {
    (void)hipStreamSynchronize(c->side_stream);
    splitk_ws_release(c->side_stream);
    (void)hipStreamDestroy(c->side_stream);
  }
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  if (c->ev_join) (void)hipEventDestroy(c->ev_join);
  for (int i = 0; i < 2; ++i) {
    if (c->d_ring[i]) (void)hipFree(c->d_ring[i]);
    if (c->ev_up[i]) (void)hipEventDestroy(c->ev_up[i]);
    if (c->ev_free[i]) (void)hipEventDestroy(c->ev_free[i]);
  }
  if (c->stream) {
    (void)hipStreamSynchronize(c->stream);
    splitk_ws_release(c->stream);
    hipStreamDestroy(c->stream);
  }
  delete c;
  return OP_OK;
}

int op_host_alloc(size_t bytes, void** p) {
  if (!p || bytes == 0) return OP_ERR_INVALID;
  *p = nullptr;
  if (hipHostMalloc(p, bytes, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    op::set_error("hipHostMalloc failed");
    return OP_ERR_HIP;
  }
  return OP_OK;
}

int op_host_free(void* p) {
  if (p && hipHostFree(p) != hipSuccess) return OP_ERR_HIP;
  return OP_OK;
}

int op_synchronize(op_ctx* c) {
  using namespace op;
  RC(check_ctx(c, false));
  OP_HIP_CHECK(hipStreamSynchronize(c->stream));
  RC(guard_check("op_synchronize"));
  return OP_OK;
}

int op_set_precision(op_ctx* c, int32_t mode) {
  using namespace op;
  RC(check_ctx(c, false));
  if (mode != OP_PRECISION_FP32 && mode != OP_PRECISION_BF16X3) {
    set_error("precision must be OP_PRECISION_FP32 or OP_PRECISION_BF16X3");
    return OP_ERR_INVALID;
  }
  c->split = mode == OP_PRECISION_BF16X3;
  return OP_OK;
}

int op_set_batch_invariant(op_ctx* c, int32_t enable) {
  using namespace op;
  RC(check_ctx(c, false));
  const int sk = enable ? 0 : 1;
  if (sk != c->splitk && c->gexec) {  // captured launches bake in the split-K choice
    OP_HIP_CHECK(hipStreamSynchronize(c->stream));
    hipGraphExecDestroy(c->gexec);
    c->gexec = nullptr;
  }
  c->splitk = sk;
  return OP_OK;
}

int op_set_peak_mode(op_ctx* c, int32_t mode, int32_t ksize) {
  using namespace op;
  RC(check_ctx(c, false));
  if (mode != OP_PEAKS_CPU_BRANCH && mode != OP_PEAKS_GPU_BRANCH) {
    set_error("op_set_peak_mode: mode must be OP_PEAKS_CPU_BRANCH or OP_PEAKS_GPU_BRANCH");
    return OP_ERR_INVALID;
  }
  if (mode == OP_PEAKS_GPU_BRANCH && (ksize < 3 || ksize > 2 * kMaxGaussR + 1 || (ksize & 1) == 0)) {
    set_error("op_set_peak_mode: ksize must be odd, 3 .. " + std::to_string(2 * kMaxGaussR + 1));
    return OP_ERR_INVALID;
  }
  OP_HIP_CHECK(hipStreamSynchronize(c->stream));
  c->peak_mode = mode;
  if (mode == OP_PEAKS_GPU_BRANCH) {
    c->gpu_r = gpu_branch_taps(c->prm.gaussian_sigma, ksize, c->gpu_taps);
  } else {
    c->gpu_r = 0;
    c->gpu_taps.clear();
  }
  const std::vector<double> gt = gauss_table(c);
  for (PostBuffers* b : {&c->pb, &c->bigb})
    if (b->gauss_w) OP_HIP_CHECK(hipMemcpy(b->gauss_w, gt.data(), gt.size() * 8, hipMemcpyHostToDevice));
  if (c->gexec) {  // captured launches bake in the peak kernel
    hipGraphExecDestroy(c->gexec);
    c->gexec = nullptr;
  }
  return OP_OK;
}

int op_set_stage_layout(op_ctx* c, int32_t planar) {
  using namespace op;
  RC(check_ctx(c, false));
  c->stage_planar = planar ? 1 : 0;
  if (c->gexec) {  // captured launches bake in the buffers
    OP_HIP_CHECK(hipStreamSynchronize(c->stream));
    hipGraphExecDestroy(c->gexec);
    c->gexec = nullptr;
  }
  return OP_OK;
}

int op_set_conv_algo(op_ctx* c, int32_t algo) {
  using namespace op;
  RC(check_ctx(c, false));
  if (algo != 0 && algo != 3 && algo != 4 && algo != 5) {
    set_error("conv algo must be 0 (per-tap gather), 3 (co-split halo), 4 (default) or 5 (default without the "
              "register-weight kernels)");
    return OP_ERR_INVALID;
  }
  c->conv_algo = algo;
  if (c->gexec) {  // captured launches bake in the kernels
    OP_HIP_CHECK(hipStreamSynchronize(c->stream));
    hipGraphExecDestroy(c->gexec);
    c->gexec = nullptr;
  }
  return OP_OK;
}

int op_get_precision(op_ctx* c, int32_t* mode) {
  using namespace op;
  RC(check_ctx(c, false));
  if (mode) *mode = c->split ? OP_PRECISION_BF16X3 : OP_PRECISION_FP32;
  return OP_OK;
}

int op_profile_enable(op_ctx* c, int32_t enable) {
  using namespace op;
  RC(check_ctx(c, false));
  c->prof = enable != 0;
  return OP_OK;
}

int op_profile_classes(op_ctx* c, int32_t mask) {
  using namespace op;
  RC(check_ctx(c, false));
  c->prof_mask = mask & ((1 << OP_PROFILE_CLASSES) - 1);
  return OP_OK;
}

int op_profile_reset(op_ctx* c) {
  using namespace op;
  RC(check_ctx(c, false));
  OP_HIP_CHECK(hipStreamSynchronize(c->stream));
  c->pending.clear();
  c->ev_used = 0;
  for (int i = 0; i < OP_PROFILE_CLASSES; ++i) {
    c->prof_ms[i] = c->prof_flops[i] = c->prof_bytes[i] = 0.0;
    c->prof_n[i] = 0;
  }
  return OP_OK;
}

int op_profile_read(op_ctx* c, int32_t cls, double* ms, int64_t* launches, double* flops, double* bytes) {
  using namespace op;
  RC(check_ctx(c, false));
  if (cls < 0 || cls >= OP_PROFILE_CLASSES) {
    set_error("profile class out of range (OP_PROFILE_CLASSES)");
    return OP_ERR_INVALID;
  }
  OP_HIP_CHECK(hipStreamSynchronize(c->stream));
  for (const ProfPair& p : c->pending) {
    float t = 0.0f;
    OP_HIP_CHECK(hipEventElapsedTime(&t, p.a, p.b));
    c->prof_ms[p.cls] += t;
    c->prof_n[p.cls] += p.n;
    c->prof_flops[p.cls] += p.flops;
    c->prof_bytes[p.cls] += p.bytes;
  }
  c->pending.clear();
  c->ev_used = 0;
  if (ms) *ms = c->prof_ms[cls];
  if (launches) *launches = c->prof_n[cls];
  if (flops) *flops = c->prof_flops[cls];
  if (bytes) *bytes = c->prof_bytes[cls];
  return OP_OK;
}

int op_last_timing(op_ctx* c, double* conv_ms, double* post_ms, double* total_ms) {
  using namespace op;
  RC(check_ctx(c, false));
  if (!c->timed) {
    set_error("no timed run (use op_run_staged)");
    return OP_ERR_STATE;
  }
  OP_HIP_CHECK(hipEventSynchronize(c->ev[2]));
  float a = 0, b = 0;
  OP_HIP_CHECK(hipEventElapsedTime(&a, c->ev[0], c->ev[1]));
  OP_HIP_CHECK(hipEventElapsedTime(&b, c->ev[1], c->ev[2]));
  if (conv_ms) *conv_ms = a;
  if (post_ms) *post_ms = b;
  if (total_ms) *total_ms = (double)a + b;
  return OP_OK;
}

}  // extern "C"

// Debugging aid (not part of the public header): copy the first `bytes` of activation buffer `id`
// (BufId order) of the current geometry to the host.
extern "C" int op_debug_read_buffer(op_ctx* c, int32_t id, void* dst, int64_t bytes) {
  using namespace op;
  RC(check_ctx(c, false));
  if (id < 0 || id >= B_COUNT || !dst || bytes < 0) return OP_ERR_INVALID;
  OP_HIP_CHECK(hipStreamSynchronize(c->stream));
  OP_HIP_CHECK(hipMemcpy(dst, c->buf[id].p, (size_t)bytes, hipMemcpyDeviceToHost));
  return OP_OK;
}
