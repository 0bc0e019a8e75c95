// Frame-parallel result gather over RCCL (SURVEY §8e, §5 "failure detection").
//
// Frames shard round-robin over one process per GPU (frame i -> rank i % world; __call__ keeps no
// cross-frame state, pose_detector.py:484-517), so the data path has no collective.  The only
// exchange is the per-frame result records, gathered to rank 0 straight from device memory:
//
//   compute stream:  ... post-process of step k -> pack_records (below) -> ev_packed[slot]
//   comm stream:     wait ev_packed[slot] -> ncclGather(records -> root) -> D2H (root, pinned)
//                    -> ev_done[slot]
//
// Two record slots, so step k's gather overlaps step k+1's forward; op_comm_wait() takes the
// oldest outstanding gather and gives up after a per-rank timeout (a stalled or dead rank): it
// aborts the communicator (ncclCommAbort) and returns OP_ERR_TIMEOUT instead of hanging.
// The communicator is created non-blocking (ncclConfig_t.blocking = 0) so initialisation obeys the
// same timeout.  Host code passes RCCL's 128-byte unique id between ranks (frames.py: TCP).
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "common.hpp"
#include "ctx.hpp"

struct op_comm {
  ncclComm_t comm = nullptr;
  int world = 0, rank = 0, device = 0;
  hipStream_t stream = nullptr;
  char* d_rec[2] = {nullptr, nullptr};  // this rank's records of one step
  char* d_all[2] = {nullptr, nullptr};  // root: every rank's records
  char* h_all[2] = {nullptr, nullptr};  // root: pinned host copy
  size_t rec_cap = 0, all_cap = 0;      // bytes per slot
  hipEvent_t ev_packed[2] = {nullptr, nullptr}, ev_done[2] = {nullptr, nullptr};
  int next = 0;                         // slot of the next submit
  int queued[2] = {0, 0};               // frames (all ranks) of an outstanding gather per slot, 0 = none
  int64_t rbytes[2] = {0, 0};
  int last = -1;                        // slot op_comm_wait returned last (op_comm_overflow*)
  int order[2] = {-1, -1};              // FIFO of outstanding slots
  bool aborted = false;
  double timeout_s = 0.0;               // op_comm_create's per-rank timeout (init and enqueue waits)
};

namespace {

using op::set_error;

int nccl_fail(const char* what, ncclResult_t r) {
  set_error(std::string(what) + ": " + ncclGetErrorString(r));
  return OP_ERR_HIP;
}

// Poll `ready` until it returns true, the communicator reports an asynchronous error, or the timeout
// expires (then abort the communicator so no RCCL kernel is left waiting on a peer).
template <class F>
int wait_for(op_comm* g, double timeout_s, const char* what, F ready) {
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    int r = ready();
    if (r == 1) return OP_OK;
    if (r < 0) return OP_ERR_HIP;
    ncclResult_t ae = ncclSuccess;
    if (g->comm && ncclCommGetAsyncError(g->comm, &ae) == ncclSuccess && ae != ncclSuccess && ae != ncclInProgress) {
      (void)ncclCommAbort(g->comm);
      g->comm = nullptr;
      g->aborted = true;
      return nccl_fail(what, ae);
    }
    const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (el > timeout_s) {
      if (g->comm) (void)ncclCommAbort(g->comm);
      g->comm = nullptr;
      g->aborted = true;
      set_error(std::string(what) + ": timed out after " + std::to_string(timeout_s) +
                " s (a rank stalled or died); communicator aborted");
      return OP_ERR_TIMEOUT;
    }
    std::this_thread::sleep_for(std::chrono::microseconds(50));
  }
}

int grow(char** p, size_t* cap, size_t bytes, bool host) {
  if (bytes <= *cap) return OP_OK;
  if (*p) {
    if (host) OP_HIP_CHECK(hipHostFree(*p));
    else OP_HIP_CHECK(hipFree(*p));
  }
  *p = nullptr;
  if (host) OP_HIP_CHECK(hipHostMalloc((void**)p, bytes, hipHostMallocDefault));
  else OP_HIP_CHECK(hipMalloc((void**)p, bytes));
  return OP_OK;
}

}  // namespace

constexpr int kKeepHdr = 5;  // int32 per frame in KeepSlot::d_hdr / h_hdr
constexpr int64_t kKeepSlotBytes = 4ll << 30;  // keep-slot map bytes per gather slot (of 288 GB HBM)
constexpr int64_t kKeepGrowBytes = 16ll << 30;  // ceiling of the grown slots' map bytes per gather slot

extern "C" {

// ---- fixed-size per-frame result records (the multi-GPU gather's payload) ----
// Record of frame i: int32 {status, n_peaks, n_persons, 0}, int64 global frame id, 8 pad bytes,
// then max_persons x 54 f64 poses and max_persons f64 scores (rows past n_persons zero).
__global__ __launch_bounds__(256) void pack_records(PostBuffers b, int first, int max_persons, int64_t frame_base,
                                                    int frame_stride, char* __restrict__ out, int64_t rec_bytes) {
  const int i = blockIdx.x;
  const int f = first + i;
  char* r = out + (int64_t)i * rec_bytes;
  const int status = b.res_hdr[4 * f];
  const int persons = status == OP_OK ? b.res_hdr[4 * f + 2] : 0;
  const int k = persons < max_persons ? persons : max_persons;
  if (threadIdx.x == 0) {
    int32_t* h = (int32_t*)r;
    h[0] = status;
    h[1] = b.res_hdr[4 * f + 1];
    h[2] = persons;
    h[3] = 0;
    *(int64_t*)(r + 16) = frame_base + (int64_t)i * frame_stride;
    *(int64_t*)(r + 24) = 0;
  }
  double* poses = (double*)(r + 32);
  double* scores = poses + (int64_t)max_persons * 54;
  const double* src = b.res_poses + (int64_t)f * b.maxs * 54;
  for (int e = threadIdx.x; e < max_persons * 54; e += 256) poses[e] = e < k * 54 ? src[e] : 0.0;
  for (int e = threadIdx.x; e < max_persons; e += 256) scores[e] = e < k ? b.res_scores[(int64_t)f * b.maxs + e] : 0.0;
}

int64_t record_bytes(int max_persons) { return 32 + (int64_t)max_persons * 55 * 8; }

// Keep slot plan (see KeepSlot; round 6): one block assigns every frame's keep
// entry in FRAME ORDER -- exclusive prefix counts over the frames before it -- so which frame goes
// without a slot when slots run short is always the same one (the last ones), whatever the block
// scheduling (the per-block atomic claims it replaces were first come, first served).  Per frame:
// why 2 (more persons than the record holds) takes page-locked rows while the rows of every earlier
// why-2 frame plus its own fit h_rows_cap, else a device res slot; why 1 (over the batched caps) a
// maps slot; a frame past `slots` such frames is not kept (where -1).
__global__ __launch_bounds__(1024) void keep_plan(PostBuffers b, int first, int n, int max_persons, int have_src,
                                                  int32_t* __restrict__ hdr, int64_t h_rows_cap, int slots) {
  __shared__ int64_t s_rows[1024];
  __shared__ int s_res[1024], s_map[1024];
  __shared__ int64_t c_rows;
  __shared__ int c_res, c_map;
  const int t = threadIdx.x;
  if (t == 0) {
    c_rows = 0;
    c_res = 0;
    c_map = 0;
  }
  for (int base = 0; base < n; base += 1024) {
    const int i = base + t;
    int status = 0, persons = 0, why = 0;
    if (i < n) {
      const int f = first + i;
      status = b.res_hdr[4 * f];
      persons = b.res_hdr[4 * f + 2];
      why = status == OP_ERR_CAPACITY ? 1 : (status == OP_OK && persons > max_persons) ? 2 : 0;
    }
    const int64_t rows = why == 2 ? (int64_t)persons * 55 : 0;
    __syncthreads();  // the carries of the previous chunk are visible, its scans are consumed
    const int64_t r0 = c_rows;
    s_rows[t] = rows;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {  // inclusive scan of the rows
      const int64_t v = t >= d ? s_rows[t - d] : 0;
      __syncthreads();
      s_rows[t] += v;
      __syncthreads();
    }
    const int64_t o = r0 + s_rows[t] - rows;  // doubles of h_rows before this frame's
    const bool in_rows = why == 2 && o + rows <= h_rows_cap;
    const int need_res = why == 2 && !in_rows, need_map = why == 1 && have_src;
    s_res[t] = need_res;
    s_map[t] = need_map;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
      const int vr = t >= d ? s_res[t - d] : 0, vm = t >= d ? s_map[t - d] : 0;
      __syncthreads();
      s_res[t] += vr;
      s_map[t] += vm;
      __syncthreads();
    }
    if (i < n) {
      int off = -1;
      if (in_rows) off = (int)o;
      else if (need_res) {
        const int sl = c_res + s_res[t] - 1;
        if (sl < slots) off = -2 - sl;
      } else if (need_map) {
        const int sl = c_map + s_map[t] - 1;
        if (sl < slots) off = sl;
      }
      int32_t* h = hdr + kKeepHdr * i;
      h[0] = status;
      h[1] = b.res_hdr[4 * (first + i) + 1];
      h[2] = status == OP_OK ? persons : 0;
      h[3] = why;
      h[4] = off;
    }
    __syncthreads();
    if (t == 1023) {
      c_rows = r0 + s_rows[1023];
      c_res += s_res[1023];
      c_map += s_map[1023];
    }
  }
}

// The frame-order plan of frame i computed by its own block (keep_overflow with plan_self, packs
// of <= kKeepSelfPlan frames): the same prefix counts as keep_plan over frames 0 .. i-1 (each block
// reads the earlier frames' headers itself: O(n^2) reads, a few microseconds at the headline's
// 232 frames) -- one launch fewer per pack, which the one-frame latency path pays for in full.
constexpr int kKeepSelfPlan = 1024;
__device__ void keep_plan_self(const PostBuffers& b, int first, int i, int max_persons, int have_src,
                               int32_t* __restrict__ hdr, int64_t h_rows_cap, int slots) {
  __shared__ int64_t r_rows[4];
  __shared__ int r_res[4], r_map[4];
  const int t = threadIdx.x;
  auto why_of = [&](int j, int* persons) {
    const int f = first + j;
    const int status = b.res_hdr[4 * f];
    *persons = b.res_hdr[4 * f + 2];
    return status == OP_ERR_CAPACITY ? 1 : (status == OP_OK && *persons > max_persons) ? 2 : 0;
  };
  // rows of every earlier why-2 frame; the earlier frames needing a res / maps slot.  A why-2 frame
  // needs a res slot iff its rows did not fit: o_j + rows_j > cap, o_j the rows of those before it
  // (rows only grow, so once one misses, every later one misses: the count of misses is the count
  // of why-2 frames j < i whose inclusive row sum exceeds the cap)
  int64_t rows = 0;
  int nres = 0, nmap = 0;
  // pass 1: inclusive row sums need order -- each thread takes a contiguous run of earlier frames
  const int per = (i + 255) / 256, j0 = min(i, t * per), j1 = min(i, j0 + per);
  int64_t run = 0;
  for (int j = j0; j < j1; ++j) {
    int p;
    if (why_of(j, &p) == 2) run += (int64_t)p * 55;
  }
  // exclusive prefix of the runs over the threads (a block scan in LDS)
  __shared__ int64_t s_run[256];
  s_run[t] = run;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const int64_t v = t >= d ? s_run[t - d] : 0;
    __syncthreads();
    s_run[t] += v;
    __syncthreads();
  }
  int64_t acc = s_run[t] - run;  // rows of the why-2 frames before this thread's run
  for (int j = j0; j < j1; ++j) {
    int p;
    const int w = why_of(j, &p);
    if (w == 2) {
      acc += (int64_t)p * 55;
      nres += acc > h_rows_cap;
    } else if (w == 1 && have_src) {
      ++nmap;
    }
  }
  rows = run;
  // block sums of the run rows (total before frame i), res and map counts
  for (int o = 32; o > 0; o >>= 1) {
    rows += __shfl_xor(rows, o);
    nres += __shfl_xor(nres, o);
    nmap += __shfl_xor(nmap, o);
  }
  if ((t & 63) == 0) {
    r_rows[t >> 6] = rows;
    r_res[t >> 6] = nres;
    r_map[t >> 6] = nmap;
  }
  __syncthreads();
  if (t == 0) {
    const int64_t o = r_rows[0] + r_rows[1] + r_rows[2] + r_rows[3];
    const int cres = r_res[0] + r_res[1] + r_res[2] + r_res[3], cmap = r_map[0] + r_map[1] + r_map[2] + r_map[3];
    int p;
    const int w = why_of(i, &p);
    const int f = first + i;
    const int status = b.res_hdr[4 * f];
    int off = -1;
    if (w == 2) {
      if (o + (int64_t)p * 55 <= h_rows_cap) off = (int)o;
      else if (cres < slots) off = -2 - cres;
    } else if (w == 1 && have_src) {
      if (cmap < slots) off = cmap;
    }
    int32_t* h = hdr + kKeepHdr * i;
    h[0] = status;
    h[1] = b.res_hdr[4 * f + 1];
    h[2] = status == OP_OK ? p : 0;
    h[3] = w;
    h[4] = off;
  }
  __syncthreads();
}

// Keep slot fill: per frame, as keep_plan (or the block itself, plan_self) assigned it.  A frame
// over the batched caps keeps its post-process input and batched peak counts (it is re-run alone in
// big mode); a frame with more persons than the record holds keeps its batched result rows (they
// are complete: copied out as they are).
__global__ __launch_bounds__(256) void keep_overflow(PostBuffers b, int first, const float* __restrict__ src,
                                                     int64_t fstride, float* __restrict__ dst, int32_t* __restrict__ cnt,
                                                     double* __restrict__ res, int32_t* __restrict__ hdr,
                                                     double* __restrict__ h_rows, int plan_self, int max_persons,
                                                     int64_t h_rows_cap, int slots) {
  const int i = blockIdx.x;
  const int f = first + i;
  if (plan_self) keep_plan_self(b, first, i, max_persons, src ? 1 : 0, hdr, h_rows_cap, slots);
  const int why = hdr[kKeepHdr * i + 3], off = hdr[kKeepHdr * i + 4];
  if (why == 2) {
    if (off == -1) return;
    const int persons = hdr[kKeepHdr * i + 2];
    const double* ps = b.res_poses + (int64_t)f * b.maxs * 54;
    const double* ss = b.res_scores + (int64_t)f * b.maxs;
    double* d = off >= 0 ? h_rows + off : res + (int64_t)(-2 - off) * b.maxs * 55;
    const int64_t sc = off >= 0 ? (int64_t)persons * 54 : (int64_t)b.maxs * 54;
    for (int e = threadIdx.x; e < persons * 54; e += 256) d[e] = ps[e];
    for (int e = threadIdx.x; e < persons; e += 256) d[sc + e] = ss[e];
    return;
  }
  if (why != 1 || !src || off < 0) return;
  if (threadIdx.x < OP_N_JOINTS) cnt[off * OP_N_JOINTS + threadIdx.x] = b.peak_cnt[f * OP_N_JOINTS + threadIdx.x];
  const float* s = src + (int64_t)f * fstride;
  float* d = dst + (int64_t)off * fstride;
  for (int64_t e = threadIdx.x; e < fstride; e += 256) d[e] = s[e];
}

}  // extern "C"

// Enqueue the records of staged frames [first, first+n) into dst (device) on the context stream;
// keep_slot 0/1 also fills that keep slot (op_comm_gather_results passes its record slot) and copies
// its headers to pinned memory on the same stream.
static int ctx_pack_records(op_ctx* c, int first, int n, int max_persons, int64_t frame_base, int frame_stride,
                            void* dst, hipStream_t* stream, int keep_slot) {
  if (first < 0 || n < 1 || first + n > c->st_n || first + n > c->pn || max_persons < 0 || keep_slot > 1) {
    set_error("pack records: bad frame range");
    return OP_ERR_INVALID;
  }
  if (keep_slot >= 0) {
    KeepSlot& k = c->keep[keep_slot];
    // page-locked rows for frames past max_persons: 256 persons per frame on average (the rest,
    // if ever, are read from the device copy in res; OP_KEEP_ROWS_AVG overrides the 256, 0 sends
    // every such frame through the device copy -- a test aid)
    const char* avg_env = getenv("OP_KEEP_ROWS_AVG");
    const int64_t avg = avg_env ? std::max(0, atoi(avg_env)) : 256;
    const int64_t want = (int64_t)n * avg * 55;
    k.rows_cap_now = std::min(want, k.h_rows_cap);
    if (want > k.h_rows_cap) {
      OP_HIP_CHECK(hipStreamSynchronize(c->stream));
      if (k.h_rows) OP_HIP_CHECK(hipHostFree(k.h_rows));
      k.h_rows = nullptr;
      k.h_rows_cap = 0;
      // coherent (fine-grained): the kernel's stores go straight to host memory
      OP_HIP_CHECK(hipHostMalloc((void**)&k.h_rows, (size_t)want * 8, hipHostMallocMapped | hipHostMallocCoherent));
      OP_HIP_CHECK(hipHostGetDevicePointer((void**)&k.d_rows_view, k.h_rows, 0));
      k.h_rows_cap = want;
      k.rows_cap_now = want;
    }
  }
  RC(profiled(c, kProfOther, 0.0, 0.0, [&] {
    hipLaunchKernelGGL(pack_records, dim3(n), dim3(256), 0, c->stream, c->pb, first, max_persons, frame_base,
                       frame_stride, (char*)dst, record_bytes(max_persons));
    OP_AFTER_LAUNCH("pack_records", c->stream);
    return OP_OK;
  }));
  if (keep_slot >= 0) {
    KeepSlot& k = c->keep[keep_slot];
    const PostRecord& r = c->post_rec;
    const float* src = r.kind == 1 ? r.low.base : r.kind == 2 ? r.full : nullptr;
    const int64_t fstride = r.kind == 1 ? r.low.fstride : r.fstride;
    const char* kf_env = getenv("OP_KEEP_FRAMES");
    const int64_t per = src ? std::max<int64_t>(1, fstride * 4) : 1;  // map bytes per kept frame
    int fit = n;  // the budget-sized count
    if (kf_env) {
      k.slots = std::min(n, std::max(1, atoi(kf_env)));
      fit = k.slots;
    } else {
      const char* kb_env = getenv("OP_KEEP_BYTES");  // test aid: the map-byte budget per gather slot
      const int64_t budget = kb_env ? std::max(0ll, atoll(kb_env)) : kKeepSlotBytes;
      fit = (int)std::min<int64_t>(n, std::max<int64_t>(8, budget / per));
      // a short gather grows the next packs' slots (`grow`), but never past kKeepGrowBytes of maps
      // (advisor r05: growth was unbounded; one gather with many over-cap frames sized every later
      // pack's slots for good, and a failed allocation then failed the pack instead of losing frames)
      const char* kg_env = getenv("OP_KEEP_GROW_BYTES");  // test aid: the growth ceiling
      const int64_t ceiling = kg_env ? std::max(0ll, atoll(kg_env)) : kKeepGrowBytes;
      const int64_t grown = std::min<int64_t>(std::max(c->keep[0].grow, c->keep[1].grow),
                                              std::max<int64_t>(8, ceiling / per));
      k.slots = (int)std::min<int64_t>(n, std::max<int64_t>(fit, grown));
    }
    // the slots' buffers; if the grown count cannot be allocated, fall back to the budget-sized one:
    // the frames beyond it travel as lost-frame statuses rather than failing the pack
    auto alloc = [&]() -> int {
      if (src) {
        RC(grow_buffer(c, (void**)&k.maps, &k.maps_cap, (size_t)k.slots * fstride * 4, "keep_maps"));
        RC(grow_buffer(c, (void**)&k.cnt, &k.cnt_cap, (size_t)k.slots * OP_N_JOINTS * 4, "keep_cnt"));
      }
      return grow_buffer(c, (void**)&k.res, &k.res_cap, (size_t)k.slots * c->pb.maxs * 55 * 8, "keep_res");
    };
    if (alloc() != OP_OK) {
      if (k.slots <= fit) return OP_ERR_HIP;
      (void)hipGetLastError();  // the failed hipMalloc's error: the smaller request below decides
      k.slots = fit;
      RC(alloc());
    }
    k.maxs = c->pb.maxs;
    const size_t hb = (size_t)n * kKeepHdr * 4;
    if (hb > k.hdr_cap) {
      OP_HIP_CHECK(hipStreamSynchronize(c->stream));
      if (k.d_hdr) OP_HIP_CHECK(hipFree(k.d_hdr));
      if (k.h_hdr) OP_HIP_CHECK(hipHostFree(k.h_hdr));
      k.d_hdr = nullptr;
      k.h_hdr = nullptr;
      k.hdr_cap = 0;
      OP_HIP_CHECK(hipMalloc((void**)&k.d_hdr, hb));
      OP_HIP_CHECK(hipHostMalloc((void**)&k.h_hdr, hb, hipHostMallocDefault));
      k.hdr_cap = hb;
    }
    RC(profiled(c, kProfOther, 0.0, 0.0, [&] {
      const char* kp_env = getenv("OP_KEEP_PLAN_KERNEL");  // test aid: 1 = the separate keep_plan launch
      const int self = n <= kKeepSelfPlan && !(kp_env && atoi(kp_env) == 1) ? 1 : 0;
      if (!self) {
        hipLaunchKernelGGL(keep_plan, dim3(1), dim3(1024), 0, c->stream, c->pb, first, n, max_persons, src ? 1 : 0,
                           k.d_hdr, k.rows_cap_now, k.slots);
        OP_AFTER_LAUNCH("keep_plan", c->stream);
      }
      hipLaunchKernelGGL(keep_overflow, dim3(n), dim3(256), 0, c->stream, c->pb, first, src, fstride, k.maps, k.cnt,
                         k.res, k.d_hdr, k.d_rows_view, self, max_persons, k.rows_cap_now, k.slots);
      OP_AFTER_LAUNCH("keep_overflow", c->stream);
      return OP_OK;
    }));
    OP_HIP_CHECK(hipMemcpyAsync(k.h_hdr, k.d_hdr, hb, hipMemcpyDeviceToHost, c->stream));
    k.rec = r;
    k.rec.s.n = n;
    if (r.kind == 1) k.rec.low.base = k.maps;
    else if (r.kind == 2) k.rec.full = k.maps;
    if (!src) k.rec.kind = 0;
    k.n = n;
  }
  OP_HIP_CHECK(hipGetLastError());
  *stream = c->stream;
  return OP_OK;
}

// This rank's frames (slot-relative) of keep slot `slot` whose record does not carry the whole
// result; valid once the slot's gather has completed (op_comm_wait).
static int ctx_kept_overflow(op_ctx* c, int slot, int32_t* frames, int32_t* reasons, int32_t cap, int32_t* count) {
  if (slot < 0 || slot > 1 || !count || (cap > 0 && !frames)) {
    set_error("kept overflow: bad arguments");
    return OP_ERR_INVALID;
  }
  KeepSlot& k = c->keep[slot];
  int m = 0, need1 = 0, need2 = 0;
  for (int i = 0; i < k.n; ++i)
    if (k.h_hdr[kKeepHdr * i + 3]) {
      if (k.h_hdr[kKeepHdr * i + 3] == 1) ++need1;
      else if (k.h_hdr[kKeepHdr * i + 4] < 0) ++need2;  // rows past the page-locked buffer
      if (m < cap) {
        frames[m] = i;
        if (reasons) reasons[m] = k.h_hdr[kKeepHdr * i + 3];
      }
      ++m;
    }
  k.grow = std::max(k.grow, std::max(need1, need2));  // the next packs keep this many
  *count = m;
  return OP_OK;
}

// Full result of frame i of keep slot `slot` (re-run alone in big mode from the kept input).
static int ctx_kept_result(op_ctx* c, int slot, int frame, double* poses, double* scores, int32_t cap,
                           op_frame_result* res) {
  if (slot < 0 || slot > 1 || !res || !poses || !scores || frame < 0 || frame >= c->keep[slot].n) {
    set_error("kept result: bad arguments");
    return OP_ERR_INVALID;
  }
  KeepSlot& k = c->keep[slot];
  memset(res, 0, sizeof(*res));
  const int32_t* hd = k.h_hdr + kKeepHdr * frame;
  if (!hd[3]) {
    set_error("kept result: the frame's record carries its whole result");
    return OP_ERR_STATE;
  }
  if (hd[3] == 2) {  // complete batched rows, kept as they were
    const int p = hd[2];
    res->status = OP_OK;
    res->n_peaks = hd[1];
    res->n_persons = p;
    if (p > cap) {
      set_error("result capacity too small");
      return OP_ERR_CAPACITY;
    }
    if (hd[4] >= 0) {  // written to page-locked memory by keep_overflow (complete: the gather waited)
      const double* h = k.h_rows + hd[4];
      memcpy(poses, h, (size_t)p * 54 * 8);
      memcpy(scores, h + (size_t)p * 54, (size_t)p * 8);
      return OP_OK;
    }
    if (hd[4] == -1) {
      set_error("kept result: more frames past max_persons than keep slots (OP_KEEP_FRAMES) in this gather");
      return OP_ERR_CAPACITY;
    }
    const double* d = k.res + (size_t)(-2 - hd[4]) * k.maxs * 55;
    OP_HIP_CHECK(hipMemcpy(poses, d, (size_t)p * 54 * 8, hipMemcpyDeviceToHost));
    OP_HIP_CHECK(hipMemcpy(scores, d + (size_t)k.maxs * 54, (size_t)p * 8, hipMemcpyDeviceToHost));
    return OP_OK;
  }
  if (k.rec.kind == 0) {
    set_error("kept result: no recorded post-process input for this slot");
    return OP_ERR_STATE;
  }
  if (hd[4] < 0) {
    set_error("kept result: more frames over the post-process caps than keep slots (OP_KEEP_FRAMES) in this gather");
    return OP_ERR_CAPACITY;
  }
  PostBuffers* B = nullptr;
  RC(rerun_big_rec(c, k.rec, hd[4], k.cnt + (size_t)hd[4] * OP_N_JOINTS, &B));
  return read_big(B, poses, scores, cap, res);
}

extern "C" {

int op_comm_unique_id(uint8_t* id) {
  if (!id) return OP_ERR_INVALID;
  static_assert(sizeof(ncclUniqueId) == OP_COMM_ID_BYTES, "ncclUniqueId size");
  ncclUniqueId u;
  ncclResult_t r = ncclGetUniqueId(&u);
  if (r != ncclSuccess) return nccl_fail("ncclGetUniqueId", r);
  memcpy(id, &u, sizeof(u));
  return OP_OK;
}

int op_comm_create(op_ctx* ctx, int32_t world, int32_t rank, const uint8_t* id, double timeout_s, op_comm** out) {
  if (!ctx || !id || !out || world < 1 || rank < 0 || rank >= world || timeout_s <= 0) {
    set_error("op_comm_create: bad arguments");
    return OP_ERR_INVALID;
  }
  *out = nullptr;
  op_comm* g = new op_comm();
  g->world = world;
  g->rank = rank;
  g->device = ctx->device;
  g->timeout_s = timeout_s;
  auto fail = [&](int rc) {
    if (g->comm) (void)ncclCommAbort(g->comm);
    if (g->stream) (void)hipStreamDestroy(g->stream);
    delete g;
    return rc;
  };
  if (hipSetDevice(g->device) != hipSuccess || hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) != hipSuccess) {
    set_error("op_comm_create: stream");
    return fail(OP_ERR_HIP);
  }
  for (int k = 0; k < 2; ++k) {
    if (hipEventCreateWithFlags(&g->ev_packed[k], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&g->ev_done[k], hipEventDisableTiming) != hipSuccess) {
      set_error("op_comm_create: events");
      return fail(OP_ERR_HIP);
    }
  }
  ncclUniqueId u;
  memcpy(&u, id, sizeof(u));
  ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
  cfg.blocking = 0;  // initialisation and collectives return at once; op_comm_wait polls with a timeout
  ncclResult_t r = ncclCommInitRankConfig(&g->comm, world, u, rank, &cfg);
  if (r != ncclSuccess && r != ncclInProgress) {
    g->comm = nullptr;
    return fail(nccl_fail("ncclCommInitRankConfig", r));
  }
  int rc = wait_for(g, timeout_s, "RCCL communicator init", [&]() -> int {
    ncclResult_t ae = ncclInProgress;
    if (ncclCommGetAsyncError(g->comm, &ae) != ncclSuccess) return -1;
    return ae == ncclSuccess ? 1 : 0;
  });
  if (rc) return fail(rc);
  *out = g;
  return OP_OK;
}

int op_comm_destroy(op_comm* g) {
  if (!g) return OP_OK;
  (void)hipSetDevice(g->device);
  if (g->stream) (void)hipStreamSynchronize(g->stream);
  if (g->comm) {
    if (g->aborted) (void)ncclCommAbort(g->comm);
    else (void)ncclCommDestroy(g->comm);
  }
  for (int k = 0; k < 2; ++k) {
    if (g->d_rec[k]) (void)hipFree(g->d_rec[k]);
    if (g->d_all[k]) (void)hipFree(g->d_all[k]);
    if (g->h_all[k]) (void)hipHostFree(g->h_all[k]);
    if (g->ev_packed[k]) (void)hipEventDestroy(g->ev_packed[k]);
    if (g->ev_done[k]) (void)hipEventDestroy(g->ev_done[k]);
  }
  if (g->stream) (void)hipStreamDestroy(g->stream);
  delete g;
  return OP_OK;
}

int op_comm_gather_results(op_comm* g, op_ctx* ctx, int32_t first, int32_t n, int32_t max_persons, int64_t frame_base,
                           int32_t frame_stride) {
  if (!g || !ctx || n < 1 || max_persons < 0) {
    set_error("op_comm_gather_results: bad arguments");
    return OP_ERR_INVALID;
  }
  if (!g->comm) {
    set_error("op_comm_gather_results: communicator aborted");
    return OP_ERR_STATE;
  }
  const int k = g->next;
  if (g->queued[k]) {
    set_error("op_comm_gather_results: two gathers outstanding; op_comm_wait first");
    return OP_ERR_STATE;
  }
  OP_HIP_CHECK(hipSetDevice(g->device));
  const int64_t rb = record_bytes(max_persons);
  const size_t mine = (size_t)n * rb, all = mine * g->world;
  if (mine > g->rec_cap || (g->rank == 0 && all > g->all_cap)) {  // grow every slot at once
    if (g->order[0] >= 0) {
      set_error("op_comm_gather_results: record size grew with a gather outstanding; op_comm_wait first");
      return OP_ERR_STATE;
    }
    OP_HIP_CHECK(hipStreamSynchronize(g->stream));
    for (int s = 0; s < 2; ++s) {
      size_t c = g->rec_cap;
      RC(grow(&g->d_rec[s], &c, mine, false));
      if (g->rank == 0) {
        c = g->all_cap;
        RC(grow(&g->d_all[s], &c, all, false));
        c = g->all_cap;
        RC(grow(&g->h_all[s], &c, all, true));
      }
    }
    g->rec_cap = std::max(g->rec_cap, mine);
    if (g->rank == 0) g->all_cap = std::max(g->all_cap, all);
  }
  // packing rewrites slot k's keep buffers (overflow headers, rows, maps): a waited-for gather in
  // that slot can no longer be queried (op_comm_overflow* then report OP_ERR_STATE, never a mix of
  // two steps' data)
  if (g->last == k) g->last = -1;
  hipStream_t cst;
  RC(ctx_pack_records(ctx, first, n, max_persons, frame_base, frame_stride, g->d_rec[k], &cst, k));
  OP_HIP_CHECK(hipEventRecord(g->ev_packed[k], cst));
  OP_HIP_CHECK(hipStreamWaitEvent(g->stream, g->ev_packed[k], 0));
  // one rank: the gather is the identity, so the root's D2H copy reads the packed records directly
  // (round 6: the one-rank ncclGather ran as an 11-us copy kernel per step)
  const bool alone = g->world == 1;
  ncclResult_t r = alone ? ncclSuccess
                         : ncclGather(g->d_rec[k], g->rank == 0 ? g->d_all[k] : nullptr, mine, ncclUint8, 0, g->comm,
                                      g->stream);
  if (r != ncclSuccess && r != ncclInProgress) return nccl_fail("ncclGather", r);
  if (r == ncclInProgress) {
    // non-blocking communicator: the gather may still be on its way into g->stream; the root's D2H
    // copy must be enqueued behind it, so wait until RCCL reports the call complete (bounded)
    RC(wait_for(g, g->timeout_s, "ncclGather enqueue", [&]() -> int {
      ncclResult_t ae = ncclInProgress;
      if (ncclCommGetAsyncError(g->comm, &ae) != ncclSuccess) return -1;
      return ae == ncclSuccess ? 1 : 0;  // an error state is reported (and aborted) by wait_for
    }));
  }
  if (g->rank == 0)
    OP_HIP_CHECK(hipMemcpyAsync(g->h_all[k], alone ? g->d_rec[k] : g->d_all[k], all, hipMemcpyDeviceToHost, g->stream));
  OP_HIP_CHECK(hipEventRecord(g->ev_done[k], g->stream));
  g->queued[k] = n * g->world;
  g->rbytes[k] = rb;
  if (g->order[0] < 0) g->order[0] = k;
  else g->order[1] = k;
  g->next = k ^ 1;
  return OP_OK;
}

int op_comm_wait(op_comm* g, double timeout_s, const void** records, int32_t* n_frames, int64_t* rec_bytes) {
  if (!g || !records || !n_frames || !rec_bytes || timeout_s <= 0) {
    set_error("op_comm_wait: bad arguments");
    return OP_ERR_INVALID;
  }
  const int k = g->order[0];
  if (k < 0) {
    set_error("op_comm_wait: no gather outstanding");
    return OP_ERR_STATE;
  }
  OP_HIP_CHECK(hipSetDevice(g->device));
  int rc = wait_for(g, timeout_s, "RCCL result gather", [&]() -> int {
    hipError_t e = hipEventQuery(g->ev_done[k]);
    if (e == hipSuccess) return 1;
    if (e == hipErrorNotReady) return 0;
    set_error(std::string("hipEventQuery: ") + hipGetErrorString(e));
    return -1;
  });
  g->order[0] = g->order[1];
  g->order[1] = -1;
  const int nf = g->queued[k];
  g->queued[k] = 0;
  if (rc) return rc;
  g->last = k;
  *records = g->rank == 0 ? g->h_all[k] : nullptr;
  *n_frames = g->rank == 0 ? nf : 0;
  *rec_bytes = g->rbytes[k];
  return OP_OK;
}

int op_comm_overflow(op_comm* g, op_ctx* ctx, int32_t* frames, int32_t* reasons, int32_t cap, int32_t* count) {
  if (!g || !ctx || !count) {
    set_error("op_comm_overflow: bad arguments");
    return OP_ERR_INVALID;
  }
  if (g->last < 0) {
    set_error("op_comm_overflow: no gather waited for yet");
    return OP_ERR_STATE;
  }
  return ctx_kept_overflow(ctx, g->last, frames, reasons, cap, count);
}

int op_comm_overflow_result(op_comm* g, op_ctx* ctx, int32_t frame, double* poses, double* scores, int32_t cap,
                            op_frame_result* res) {
  if (!g || !ctx) {
    set_error("op_comm_overflow_result: bad arguments");
    return OP_ERR_INVALID;
  }
  if (g->last < 0) {
    set_error("op_comm_overflow_result: no gather waited for yet");
    return OP_ERR_STATE;
  }
  OP_HIP_CHECK(hipSetDevice(g->device));
  return ctx_kept_result(ctx, g->last, frame, poses, scores, cap, res);
}


int op_pack_results(op_ctx* c, int32_t first, int32_t n, int32_t max_persons, int64_t frame_base, int32_t frame_stride,
                    void* host_records) {
  using namespace op;
  RC(check_ctx(c, false));
  if (!host_records) {
    set_error("op_pack_results: null output");
    return OP_ERR_INVALID;
  }
  const size_t bytes = (size_t)n * record_bytes(max_persons);
  RC(ensure_scratch(c, bytes));
  hipStream_t st;
  RC(ctx_pack_records(c, first, n, max_persons, frame_base, frame_stride, c->d_scratch, &st, -1));
  OP_HIP_CHECK(hipMemcpyAsync(host_records, c->d_scratch, bytes, hipMemcpyDeviceToHost, st));
  OP_HIP_CHECK(hipStreamSynchronize(st));
  return OP_OK;
}

}  // extern "C"
