// Frame staging and upload, the single-scale staged run (eager and as a captured graph) and
// op_detect.
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "common.hpp"
#include "ctx.hpp"

namespace op {

// Pack planar (n, 57, lh, lw) maps [38 paf | 19 heat] into an NHWC (n, lh, lw, 57) device buffer.
int stage_maps_dev(op_ctx* c, const float* maps, int n, int lh, int lw, float** out) {
  using namespace op;
  c->post_rec.kind = 0;  // staged maps are replaced
  const size_t fl = (size_t)n * 57 * lh * lw;
  std::vector<float> t(fl);
  for (int f = 0; f < n; ++f)
    for (int ch = 0; ch < 57; ++ch)
      for (int y = 0; y < lh; ++y)
        for (int x = 0; x < lw; ++x)
          t[(((size_t)f * lh + y) * lw + x) * 57 + ch] = maps[(((size_t)f * 57 + ch) * lh + y) * lw + x];
  RC(grow_buffer(c, (void**)&c->d_maps, &c->maps_bytes, fl * 4, "maps"));
  // the null-stream copy is not ordered against the (non-blocking) compute stream: a queued run may
  // still read the old maps
  OP_HIP_CHECK(hipStreamSynchronize(c->stream));
  OP_HIP_CHECK(hipMemcpy(c->d_maps, t.data(), fl * 4, hipMemcpyHostToDevice));
  *out = c->d_maps;
  return OP_OK;
}

// A pending op_upload_frames becomes the staged frame set: the compute stream waits for its copy
// and moves the ring slot into d_frames (the buffer kernels and captured graphs read).
int take_upload(op_ctx* c) {
  if (c->up_slot < 0) return OP_OK;
  const int k = c->up_slot;
  c->up_slot = -1;
  const size_t bytes = (size_t)c->up_n * c->up_h * c->up_w * 3;
  RC(grow_buffer(c, (void**)&c->d_frames, &c->frames_bytes, bytes, "frames"));
  OP_HIP_CHECK(hipStreamWaitEvent(c->stream, c->ev_up[k], 0));
  OP_HIP_CHECK(hipMemcpyAsync(c->d_frames, c->d_ring[k], bytes, hipMemcpyDeviceToDevice, c->stream));
  OP_HIP_CHECK(hipEventRecord(c->ev_free[k], c->stream));
  if (c->st_n != c->up_n || c->st_h != c->up_h || c->st_w != c->up_w) {
    if (c->gexec) {
      OP_HIP_CHECK(hipStreamSynchronize(c->stream));
      hipGraphExecDestroy(c->gexec);
      c->gexec = nullptr;
    }
  }
  c->st_n = c->up_n;
  c->st_h = c->up_h;
  c->st_w = c->up_w;
  return OP_OK;
}

// network input / post-process map size of the staged results (single scale or precise)
void staged_sizes(op_ctx* c, int* in_w, int* in_h, int* map_w, int* map_h) {
  if (c->st_precise) {
    *in_w = c->st_net_w;
    *in_h = c->st_net_h;
    *map_w = c->st_w;
    *map_h = c->st_h;
    return;
  }
  optimal_size(c->st_h, c->st_w, c->prm.inference_img_size, 8, in_w, in_h);
  optimal_size(c->st_h, c->st_w, c->prm.heatmap_size, 8, map_w, map_h);
}

int staged_range(op_ctx* c, const char* who, int32_t first, int32_t n) {
  if (c->st_n < 1) {
    set_error(std::string(who) + ": no staged frames");
    return OP_ERR_STATE;
  }
  if (first < 0 || first > c->st_n - n)
    return invalid(who, "first, n: frames " + std::to_string(first) + " .. " + std::to_string((int64_t)first + n - 1) +
                            " are outside the " + std::to_string(c->st_n) + " staged frames");
  return OP_OK;
}

// One frame (h x w x 3 u8, row stride row_stride) from caller memory into d_frames on the compute
// stream, through the context's page-locked staging buffer (op_detect / op_detect_precise).
int upload_one_frame(op_ctx* c, const uint8_t* bgr, int h, int w, int64_t row_stride) {
  const size_t row = (size_t)w * 3, bytes = row * h;
  RC(grow_buffer(c, (void**)&c->d_frames, &c->frames_bytes, bytes, "frames"));
  OP_HIP_CHECK(hipStreamSynchronize(c->stream));  // the staging buffer's previous copy has completed
  if (bytes > c->up_pinned_bytes) {
    if (c->up_pinned) OP_HIP_CHECK(hipHostFree(c->up_pinned));
    c->up_pinned = nullptr;
    c->up_pinned_bytes = 0;
    OP_HIP_CHECK(hipHostMalloc((void**)&c->up_pinned, bytes, hipHostMallocDefault));
    c->up_pinned_bytes = bytes;
  }
  for (int y = 0; y < h; ++y) memcpy(c->up_pinned + (size_t)y * row, bgr + (size_t)y * row_stride, row);
  OP_HIP_CHECK(hipMemcpyAsync(c->d_frames, c->up_pinned, bytes, hipMemcpyHostToDevice, c->stream));
  return OP_OK;
}

int stage_reserve(op_ctx* c, size_t bytes) {
  c->up_slot = -1;  // a pending op_upload_frames is replaced
  return grow_buffer(c, (void**)&c->d_frames, &c->frames_bytes, bytes, "frames");
}

int stage_commit(op_ctx* c, int n, int h, int w) {
  if (c->st_n != n || c->st_h != h || c->st_w != w) {
    if (c->gexec) {
      hipGraphExecDestroy(c->gexec);
      c->gexec = nullptr;
    }
  }
  c->st_n = n;
  c->st_h = h;
  c->st_w = w;
  return OP_OK;
}

}  // namespace op

extern "C" {

// Enqueue preprocess + forward + post-process for the staged batch on the context stream.
static int enqueue_staged(op_ctx* c, bool timing) {
  c->st_precise = false;
  using namespace op;
  int in_w, in_h, map_w, map_h;
  optimal_size(c->st_h, c->st_w, c->prm.inference_img_size, 8, &in_w, &in_h);
  optimal_size(c->st_h, c->st_w, c->prm.heatmap_size, 8, &map_w, &map_h);
  RC(ensure_geometry(c, c->st_n, in_h, in_w));
  RC(ensure_post(c, c->st_n, map_h, map_w));
  if (timing) OP_HIP_CHECK(hipEventRecord(c->ev[0], c->stream));
  if (c->split) {  // the network input is resampled inside the conv1_1 kernel
    RC(run_forward(c, c->d_frames, (int64_t)c->st_h * c->st_w * 3, (int64_t)c->st_w * 3, c->st_h, c->st_w));
  } else {
    RC(profiled(c, kProfInput, 0.0, 0.0, [&] {
      return launch_preprocess(c->d_frames, (int64_t)c->st_h * c->st_w * 3, (int64_t)c->st_w * 3, c->st_n, c->st_h,
                               c->st_w, in_h, in_w, c->buf[B_X0].p, c->stream);
    }));
    RC(run_forward(c));
  }
  if (timing) OP_HIP_CHECK(hipEventRecord(c->ev[1], c->stream));
  const int lh = in_h / 8, lw = in_w / 8;
  MapSource src;
  if (c->use_maps) {
    if (c->sm_n < c->st_n || c->sm_h != lh || c->sm_w != lw) {
      set_error("staged maps do not match the staged frames (n, h/8, w/8)");
      return OP_ERR_STATE;
    }
    src = MapSource{c->d_maps, (int64_t)57 * lh * lw, 0, 57, 0, 38};
  } else if (c->split) {
    const Act& m = c->buf[B_MAP32];
    src = MapSource{m.p, (int64_t)m.frame_floats(), 0, m.cs, 0, 40};
  } else {
    const Act& cat = c->buf[B_CAT];
    src = MapSource{cat.p, (int64_t)cat.frame_floats(), cat.pad, cat.cs, kCatPaf, kCatHeat};
  }
  PostShape s;
  post_shape(c, s, c->st_n, lh, lw, map_h, map_w, (double)map_w, (double)c->st_w / map_w, (double)c->st_h / map_h);
  // post-process algorithmic HBM bytes: 57-ch low-res read + 18-ch upsample write +
  // 2 x (read + write) Gaussian passes + NMS read, f32
  const double mp = (double)c->st_n * map_h * map_w;
  const double pbytes = 4.0 * ((double)c->st_n * 57 * lh * lw + 18 * mp + 2 * 2 * 18 * mp + 18 * mp);
  post_record(c, 1, &src, nullptr, 0, s);
  RC(profiled(c, kProfPost, 0.0, pbytes, [&] { return launch_post_maps(src, s, c->pb, c->stream); }));
  if (timing) OP_HIP_CHECK(hipEventRecord(c->ev[2], c->stream));
  c->timed = timing;
  return OP_OK;
}

int op_stage_frames(op_ctx* c, const uint8_t* frames, int32_t n, int32_t h, int32_t w) {
  using namespace op;
  RC(check_ctx(c, false));
  if (!frames || n < 1 || h < 8 || w < 8) {
    set_error("op_stage_frames: bad arguments");
    return OP_ERR_INVALID;
  }
  const size_t bytes = (size_t)n * h * w * 3;
  RC(stage_reserve(c, bytes));
  OP_HIP_CHECK(hipMemcpyAsync(c->d_frames, frames, bytes, hipMemcpyHostToDevice, c->stream));
  OP_HIP_CHECK(hipStreamSynchronize(c->stream));
  return stage_commit(c, n, h, w);
}

int op_stage_maps(op_ctx* c, const float* maps, int32_t n, int32_t mh, int32_t mw) {
  using namespace op;
  RC(check_ctx(c, false));
  if (!maps || n < 1 || mh < 2 || mw < 2) {
    set_error("op_stage_maps: bad arguments");
    return OP_ERR_INVALID;
  }
  if (c->st_n > 0 && mh == c->st_h && mw == c->st_w) {
    // full-resolution maps of the staged frames: the precise post-process input (kept planar)
    const size_t bytes = (size_t)n * 57 * mh * mw * 4;
    c->post_rec.kind = 0;  // staged maps are replaced
    RC(grow_buffer(c, (void**)&c->d_fmaps, &c->fmaps_bytes, bytes, "full_maps"));
    OP_HIP_CHECK(hipStreamSynchronize(c->stream));  // a queued precise run may still read the old maps
    OP_HIP_CHECK(hipMemcpy(c->d_fmaps, maps, bytes, hipMemcpyHostToDevice));
    c->fm_n = n;
    c->fm_h = mh;
    c->fm_w = mw;
  } else {
    float* dm;
    RC(stage_maps_dev(c, maps, n, mh, mw, &dm));
    c->sm_n = n;
    c->sm_h = mh;
    c->sm_w = mw;
  }
  if (c->gexec) {
    hipGraphExecDestroy(c->gexec);
    c->gexec = nullptr;
  }
  return OP_OK;
}

int op_use_staged_maps(op_ctx* c, int32_t enable) {
  if (!c) return OP_ERR_INVALID;
  c->use_maps = enable != 0;
  if (c->gexec) {
    hipGraphExecDestroy(c->gexec);
    c->gexec = nullptr;
  }
  return OP_OK;
}

int op_upload_frames(op_ctx* c, const uint8_t* frames, int32_t n, int32_t h, int32_t w) {
  using namespace op;
  RC(check_ctx(c, false));
  if (!frames || n < 1 || h < 8 || w < 8) {
    set_error("op_upload_frames: bad arguments");
    return OP_ERR_INVALID;
  }
  if (!c->copy_stream) {
    OP_HIP_CHECK(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) {
      OP_HIP_CHECK(hipEventCreateWithFlags(&c->ev_up[i], hipEventDisableTiming));
      OP_HIP_CHECK(hipEventCreateWithFlags(&c->ev_free[i], hipEventDisableTiming));
    }
  }
  RC(take_upload(c));  // an upload never run is still staged: this one replaces it afterwards
  const int k = c->ring_next;
  const size_t bytes = (size_t)n * h * w * 3;
  if (bytes > c->ring_bytes[k]) {
    OP_HIP_CHECK(hipStreamSynchronize(c->copy_stream));
    OP_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (c->d_ring[k]) OP_HIP_CHECK(hipFree(c->d_ring[k]));
    c->d_ring[k] = nullptr;
    OP_HIP_CHECK(hipMalloc((void**)&c->d_ring[k], bytes));
    c->ring_bytes[k] = bytes;
  }
  // the slot's previous frames must have been moved out by the compute stream first
  OP_HIP_CHECK(hipStreamWaitEvent(c->copy_stream, c->ev_free[k], 0));
  OP_HIP_CHECK(hipMemcpyAsync(c->d_ring[k], frames, bytes, hipMemcpyHostToDevice, c->copy_stream));
  OP_HIP_CHECK(hipEventRecord(c->ev_up[k], c->copy_stream));
  c->up_slot = k;
  c->up_n = n;
  c->up_h = h;
  c->up_w = w;
  c->ring_next = k ^ 1;
  return OP_OK;
}

int op_upload_wait(op_ctx* c) {
  using namespace op;
  RC(check_ctx(c, false));
  for (int k = 0; k < 2; ++k)
    if (c->ev_up[k]) OP_HIP_CHECK(hipEventSynchronize(c->ev_up[k]));
  return OP_OK;
}

int op_run_staged(op_ctx* c) {
  using namespace op;
  RC(check_ctx(c, true));
  RC(take_upload(c));
  if (c->st_n < 1) {
    set_error("no staged frames");
    return OP_ERR_STATE;
  }
  return enqueue_staged(c, true);
}

int op_run_staged_graph(op_ctx* c) {
  using namespace op;
  RC(check_ctx(c, true));
  RC(take_upload(c));
  if (c->st_n < 1) {
    set_error("no staged frames");
    return OP_ERR_STATE;
  }
  // geometry/buffers must exist before capture (allocation and memsets are not captured)
  int in_w, in_h, map_w, map_h;
  optimal_size(c->st_h, c->st_w, c->prm.inference_img_size, 8, &in_w, &in_h);
  optimal_size(c->st_h, c->st_w, c->prm.heatmap_size, 8, &map_w, &map_h);
  RC(ensure_geometry(c, c->st_n, in_h, in_w));
  RC(ensure_post(c, c->st_n, map_h, map_w));
  // the graph bakes in every pointer and size: replay only if none changed since capture
  const uintptr_t key[10] = {(uintptr_t)c->st_n, (uintptr_t)c->st_h, (uintptr_t)c->st_w, (uintptr_t)c->use_maps,
                             (uintptr_t)c->arena, (uintptr_t)c->post_arena, (uintptr_t)c->d_frames,
                             (uintptr_t)c->d_maps, (uintptr_t)c->gn, (uintptr_t)(c->gh * 65536 + c->gw) * 4 + (uintptr_t)c->split * 2 + (uintptr_t)c->splitk};
  if (c->gexec && memcmp(key, c->g_key, sizeof(key)) != 0) {
    hipGraphExecDestroy(c->gexec);
    c->gexec = nullptr;
  }
  if (!c->gexec) {
    OP_HIP_CHECK(hipStreamSynchronize(c->stream));
    memcpy(c->g_key, key, sizeof(key));
    const bool prof = c->prof;
    c->prof = false;  // no event records inside the capture
    if (c->graph) {
      hipGraphDestroy(c->graph);
      c->graph = nullptr;
    }
    hipGraph_t g = nullptr;
    for (int attempt = 0;; ++attempt) {
      OP_HIP_CHECK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
      int rc = enqueue_staged(c, false);
      hipError_t e = hipStreamEndCapture(c->stream, &g);
      if (rc || e != hipSuccess) {
        c->prof = prof;
        if (g) hipGraphDestroy(g);
        if (rc) return rc;
        OP_HIP_CHECK(e);
      }
      // a split-K launch that found its workspace too small during capture ran unsplit: grow the
      // workspace outside capture and capture again, so replays match eager runs
      if (splitk_ws_capture_short(c->stream) == 0) break;
      hipGraphDestroy(g);
      g = nullptr;
      if (attempt > 0 || splitk_ws_reserve(c->stream) != 0) {
        c->prof = prof;
        set_error("split-K workspace allocation failed");
        return OP_ERR_HIP;
      }
    }
    c->prof = prof;
    c->graph = g;
    OP_HIP_CHECK(hipGraphInstantiate(&c->gexec, g, nullptr, nullptr, 0));
    if (const char* d = getenv("OP_GRAPH_DUMP")) {  // debugging aid: DOT dump of every captured graph
      static int seq = 0;
      const std::string path = std::string(d) + "/graph_" + std::to_string(seq++) + ".dot";
      hipGraphDebugDotPrint(g, path.c_str(), hipGraphDebugDotFlagsVerbose);
    }
  }
  if (getenv("OP_GRAPH_DRYRUN")) return enqueue_staged(c, false);  // debugging aid: eager instead of replay
  OP_HIP_CHECK(hipGraphLaunch(c->gexec, c->stream));
  c->timed = false;
  return OP_OK;
}

static bool host_side(const void* p) {
  if (!p) return false;
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();  // unregistered (pageable) host memory
    return true;
  }
  return a.type != hipMemoryTypeDevice;
}

int op_graph_info(op_ctx* c, int32_t* nodes, int32_t* kernels, int32_t* memsets, int32_t* memcpys,
                  int32_t* host_nodes) {
  using namespace op;
  RC(check_ctx(c, false));
  if (!nodes || !kernels || !memsets || !memcpys || !host_nodes) {
    set_error("op_graph_info: null output");
    return OP_ERR_INVALID;
  }
  if (!c->graph) {
    set_error("op_graph_info: no captured graph");
    return OP_ERR_STATE;
  }
  size_t n = 0;
  OP_HIP_CHECK(hipGraphGetNodes(c->graph, nullptr, &n));
  std::vector<hipGraphNode_t> v(n);
  OP_HIP_CHECK(hipGraphGetNodes(c->graph, v.data(), &n));
  *nodes = (int32_t)n;
  *kernels = *memsets = *memcpys = *host_nodes = 0;
  for (hipGraphNode_t nd : v) {
    hipGraphNodeType t;
    OP_HIP_CHECK(hipGraphNodeGetType(nd, &t));
    if (t == hipGraphNodeTypeKernel) {
      ++*kernels;
    } else if (t == hipGraphNodeTypeMemset) {
      hipMemsetParams mp;
      OP_HIP_CHECK(hipGraphMemsetNodeGetParams(nd, &mp));
      ++*memsets;
      if (host_side(mp.dst)) ++*host_nodes;
    } else if (t == hipGraphNodeTypeMemcpy) {
      hipMemcpy3DParms mp;
      OP_HIP_CHECK(hipGraphMemcpyNodeGetParams(nd, &mp));
      ++*memcpys;
      const void* src = mp.srcArray ? nullptr : mp.srcPtr.ptr;
      const void* dst = mp.dstArray ? nullptr : mp.dstPtr.ptr;
      if (mp.kind == hipMemcpyHostToDevice || mp.kind == hipMemcpyDeviceToHost || mp.kind == hipMemcpyHostToHost ||
          host_side(src) || host_side(dst))
        ++*host_nodes;
    } else if (t != hipGraphNodeTypeEmpty) {
      ++*host_nodes;  // host callbacks, event records / waits, child graphs: not expected
    }
  }
  return OP_OK;
}

int op_detect(op_ctx* c, const uint8_t* bgr, int32_t h, int32_t w, int64_t row_stride, double* poses, double* scores,
              int32_t cap, op_frame_result* res) {
  using namespace op;
  RC(check_ctx(c, true));
  if (!bgr || !res || h < 8 || w < 8 || row_stride < (int64_t)w * 3) {
    set_error("op_detect: bad arguments");
    return OP_ERR_INVALID;
  }
  c->up_slot = -1;  // a pending op_upload_frames is replaced
  RC(upload_one_frame(c, bgr, h, w, row_stride));
  c->st_n = 1;
  c->st_h = h;
  c->st_w = w;
  const bool keep_maps = c->use_maps;
  c->use_maps = false;
  int rc = enqueue_staged(c, false);
  c->use_maps = keep_maps;
  if (rc) return rc;
  OP_HIP_CHECK(hipStreamSynchronize(c->stream));
  RC(guard_check("op_detect"));
  return op_fetch_result(c, 0, poses, scores, cap, res);
}

}  // extern "C"
