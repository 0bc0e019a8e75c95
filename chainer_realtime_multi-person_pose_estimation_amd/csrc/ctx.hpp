// The library's internal context: struct op_ctx (one context = one device, one stream, weights packed
// once in HBM, an activation arena carved per (batch, net size) geometry, and the post-process
// buffers), the host-side types it is made of, and the helpers that cross the host units
// (runtime.hip, weights.hip, forward.hip, post_api.hip, staged.hip, gather.hip, precise.hip).
// Kernel-only units include common.hpp alone.
#pragma once
#include <vector>

#include "common.hpp"

namespace op {

// ---- packed weights ----
struct PackedConv {
  float* w = nullptr;
  float* b = nullptr;
  int cop = 0, cin_phys = 0, ks = 0;
  int cin_log = 0, co_log = 0;  // logical (reference) channel counts, for algorithmic FLOPs
  void* ws = nullptr;           // 3xBF16 split weights [c16][tap][cop][k-half][hi8 lo8]
  int cin16 = 0;                // input channels padded to 16 (split path)
};

struct ProfPair {
  int cls;
  hipEvent_t a, b;
  double flops, bytes;
  int n;  // launches between a and b (a joined run of back-to-back launches of one class)
};

// ---- activation buffers ----
struct Act {
  float* p = nullptr;
  int pad = 0, cs = 0, h = 0, w = 0;
  int planar = 0;  // split layout: 0 [frame][hp][wp][cs], 1 chunk-planar (SplitConvShape::in_planar)
  size_t frame_floats() const { return (size_t)(h + 2 * pad) * (w + 2 * pad) * cs; }
};

// Input of the last batched post-process (0: none, 1: low-res maps through the fused upsample,
// 2: full-resolution planar maps of the precise path), kept so one frame can be re-run uncapped.
struct PostRecord {
  int kind = 0;
  MapSource low{};
  const float* full = nullptr;
  int64_t fstride = 0;
  PostShape s{};
};

// Per gather slot (gather.hip's two record slots): the post-process input of the frames whose
// record cannot carry the whole result (over the batched caps, or more persons than the record
// holds), copied aside on the device when the records are packed, so the owning rank can re-run
// them after the next step has overwritten the batched buffers (op_comm_overflow*).
struct KeepSlot {
  // kept frames are compacted into `slots` entries assigned by device counters.  Round 5 (advisor
  // r04): every frame of the pack gets a slot while their maps fit kKeepSlotBytes (the 368x368 maps
  // of 232 frames: 125 MB; 16 precise 1280x720 frames: 3.4 GB), at least 8 beyond that, and a
  // gather that had more overflow frames than slots grows the next packs' slots (`grow`);
  // OP_KEEP_FRAMES=<n> pins the count (test aid).  A frame left without a slot is reported as a
  // frame status through the overflow exchange (frames.py), never as an exception before it
  float* maps = nullptr;  // [slot][fstride] post-process input of frames over the batched caps
  size_t maps_cap = 0;  // bytes
  double* res = nullptr;  // [slot][maxs][54 + 1] rows of frames past max_persons not in h_rows
  size_t res_cap = 0;
  int slots = 0;
  int maxs = 0;
  int32_t* cnt = nullptr;
  size_t cnt_cap = 0;
  // n x kKeepHdr {status, n_peaks, n_persons, why: 0 whole record, 1 over the caps, 2 > max_persons,
  // where: why 1: its maps / cnt slot; why 2: >= 0 offset of its rows in h_rows (doubles), <= -2
  // res slot -2 - where; -1: not kept (more such frames than slots: OP_ERR_CAPACITY on collection)}
  int32_t* d_hdr = nullptr;
  int32_t* h_hdr = nullptr;  // pinned copy, complete when the slot's gather is
  size_t hdr_cap = 0;
  // rows of the frames past max_persons written by keep_overflow straight into page-locked host
  // memory (poses then scores per frame, packed by a device counter), so collecting them needs no
  // GPU copy: a copy on any stream would share a hardware queue with the next steps' compute
  // and wait for them (round 3: 65 ms per 114-frame step on the network-maps line)
  double* h_rows = nullptr;
  double* d_rows_view = nullptr;  // the device's address of h_rows (hipHostGetDevicePointer)
  int64_t h_rows_cap = 0;  // doubles
  int64_t rows_cap_now = 0;  // of them, usable by the current pack (OP_KEEP_ROWS_AVG)
  PostRecord rec{};
  int n = 0;
  int grow = 0;  // overflow frames of the largest gather seen that needed a slot
};

enum BufId {
  B_X0, B_C11, B_C12, B_P1, B_C21, B_C22, B_P2, B_C3A, B_C3B, B_C34, B_P3, B_C41, B_C42, B_C43, B_CAT, B_BRA, B_BRB,
  B_S1, B_MAP32, B_PA, B_PB, B_CATP, B_COUNT
};

// their names (the guard bands report them)
static const char* const kBufName[B_COUNT] = {"X0",  "C11", "C12", "P1",  "C21", "C22", "P2",  "C3A", "C3B", "C34",
                                              "P3",  "C41", "C42", "C43", "CAT", "BRA", "BRB", "S1",  "MAP32",
                                              "PA",  "PB",  "CATP"};

// the op_profile_read classes after the three conv classes (openpose_hip.h; forward.hip conv_class)
constexpr int kProfPost = 3, kProfInput = 4, kProfMapResize = 5, kProfOther = 6;

}  // namespace op

using namespace op;  // the host units (the only includers) name op's types unqualified, as op_ctx does

struct op_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  op_params prm;
  op_limits lim;
  bool have_weights = false;
  // packed convolutions (see build_weights)
  PackedConv bb[12];           // backbone conv1_1 .. conv4_4_CPM
  PackedConv s1_first;         // conv5_1 L1|L2 fused (Co 256)
  PackedConv s1_g[2][3];       // [branch][conv5_2, conv5_3, conv5_4]
  PackedConv s1_last[2];       // conv5_5 L1 / L2
  PackedConv st_first[5];      // Mconv1 stage s, fused (Co 256, 192 phys in)
  PackedConv st_g[5][2][5];    // [stage][branch][Mconv2..Mconv6]
  PackedConv st_last[5][2];    // Mconv7
  float* w11 = nullptr;        // conv1_1 weights [tap][ci][co] f32 for the VALU kernel (conv11.hip)
  // activation arena of the current geometry, and every geometry's arena (multi-scale: one per
  // scale, kept so switching scales needs neither an allocation nor a re-zeroing memset)
  void* arena = nullptr;
  size_t arena_bytes = 0;
  struct GeomArena {
    int n, h, w;
    bool split;
    void* p;
    size_t bytes;
    uint64_t used;
  };
  std::vector<GeomArena> arenas;
  uint64_t arena_clock = 0;
  int gn = 0, gh = 0, gw = 0;  // current geometry (batch, net h, net w)
  bool split = true;           // 3xBF16 split convs (default) or exact f32 MFMA convs
  bool gsplit = true;          // format the arena is currently carved for
  int conv_algo = 4;           // split-path conv kernel family (op_set_conv_algo)
  int stage_planar = 1;        // chunk-planar 7x7 stage tensors where conv_m16 takes them (op_set_stage_layout)
  Act buf[B_COUNT];
  // post-process
  PostBuffers pb{};
  void* post_arena = nullptr;
  size_t post_bytes = 0;
  int pn = 0, pmh = 0, pmw = 0;  // post geometry
  std::vector<double> gauss_host;
  int gauss_r = 0;
  // op_set_peak_mode: 1 = the reference's GPU-branch peaks (ksize x ksize unnormalised Gaussian,
  // zero padding, >= NMS) in the single-scale post-process; gpu_taps = its 1-D factor (2 gpu_r + 1)
  int peak_mode = 0;
  int gpu_r = 0;
  std::vector<double> gpu_taps;
  // staging
  uint8_t* d_frames = nullptr;
  size_t frames_bytes = 0;
  // async frame uploads (op_upload_frames): a 2-slot device ring filled on copy_stream; the next
  // run waits for its slot's copy and moves it into d_frames on the compute stream
  hipStream_t copy_stream = nullptr;
  // detect_precise (round 6): the small scales' forwards run on side_stream, concurrent with the large
  // ones on the compute stream (fork / join events); while they are enqueued `stream` points at it
  hipStream_t side_stream = nullptr;
  hipStream_t main_stream = nullptr;  // the compute stream while `stream` is swapped to side_stream
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  uint8_t* d_ring[2] = {nullptr, nullptr};
  size_t ring_bytes[2] = {0, 0};
  hipEvent_t ev_up[2] = {nullptr, nullptr}, ev_free[2] = {nullptr, nullptr};
  int ring_next = 0, up_slot = -1, up_n = 0, up_h = 0, up_w = 0;
  int st_n = 0, st_h = 0, st_w = 0;
  bool st_precise = false;     // the staged results come from op_run_staged_precise
  int st_net_w = 0, st_net_h = 0;
  float* d_maps = nullptr;
  size_t maps_bytes = 0;
  int sm_n = 0, sm_h = 0, sm_w = 0;
  float* d_fmaps = nullptr;  // staged full-resolution maps for the precise post-process, planar (n, 57, h, w)
  size_t fmaps_bytes = 0;
  int fm_n = 0, fm_h = 0, fm_w = 0;
  bool use_maps = false;
  float* d_scratch = nullptr;
  size_t scratch_bytes = 0;
  // timing
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  bool timed = false;
  // per-class launch profiling
  bool prof = false;
  int splitk = 1;  // op_set_batch_invariant(0): small 7x7 launches may split K
  int prof_mask = 0x7F;  // kernel classes timed while prof (op_profile_classes)
  // set by the forward around launches it issues back to back (the 7x7 Mconv1..Mconv5 of a stage):
  // a profiled launch then extends the previous pair of its class instead of adding an event pair
  // (an event record between two kernels costs ~10 us of stream idle time on this runtime)
  bool prof_join = false;
  std::vector<hipEvent_t> ev_pool;
  size_t ev_used = 0;
  std::vector<op::ProfPair> pending;
  double prof_ms[OP_PROFILE_CLASSES] = {}, prof_flops[OP_PROFILE_CLASSES] = {}, prof_bytes[OP_PROFILE_CLASSES] = {};
  int64_t prof_n[OP_PROFILE_CLASSES] = {};
  // graph
  hipGraphExec_t gexec = nullptr;
  hipGraph_t graph = nullptr;
  uintptr_t g_key[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  // multi-scale path: per-scale map intermediates and the running sums over scales
  float* d_pmid = nullptr;
  size_t pmid_bytes = 0;
  float* d_psum = nullptr;
  size_t psum_bytes = 0;
  // pinned host staging for batched result fetches
  char* host_stage = nullptr;
  size_t host_stage_bytes = 0;
  // pinned host staging for the one-frame uploads of op_detect / op_detect_precise: the caller's
  // (pageable, possibly row-strided) image is packed here by the host and copied with one plain
  // async copy on the compute stream -- no pageable or 2D copy path of the HIP runtime is involved
  uint8_t* up_pinned = nullptr;
  size_t up_pinned_bytes = 0;
  // op_jpeg_stage: the page-locked staging of a batch ([frame table | coefficient blocks | frames
  // given as pixels]) and its device side ([frame table | coefficient blocks | component planes])
  uint8_t* jpeg_pinned = nullptr;
  size_t jpeg_pinned_bytes = 0;
  uint8_t* d_jpeg = nullptr;
  size_t jpeg_bytes = 0;
  // uncapped post-process: the last batched post-process's input (to re-run one frame) and the
  // one-frame big-mode buffers sized from that frame's own counts
  op::PostRecord post_rec;
  op::KeepSlot keep[2];
  PostBuffers bigb{};
  void* bb_arena = nullptr;
  int big_frame = -1;  // frame of post_rec whose big-mode result sits in bb
};

#define RC(x)            \
  do {                   \
    int _r = (x);        \
    if (_r) return _r;   \
  } while (0)

namespace op {

extern size_t g_guard;  // OP_GUARD bytes after every device buffer (runtime.hip)

// ---- helpers that cross the host units, by the unit that defines them (hidden: they are not part
// of the library's interface and stay out of its dynamic symbols) ----
#pragma GCC visibility push(hidden)
// runtime.hip
void guard_add(const char* name, void* p, hipStream_t st);
void guard_forget(const void* base, size_t bytes);
int guard_check(const char* where);
int grow_buffer(op_ctx* c, void** p, size_t* cap, size_t bytes, const char* name);
int ensure_scratch(op_ctx* c, size_t bytes);
hipEvent_t pool_event(op_ctx* c);
int check_ctx(op_ctx* c, bool need_weights);
void free_weights(op_ctx* c);
// forward.hip
int ensure_geometry(op_ctx* c, int n, int h, int w);
int run_forward(op_ctx* c, const uint8_t* frames = nullptr, int64_t frame_bytes = 0, int64_t row_stride = 0,
                int sh = 0, int sw = 0, float* stages = nullptr, int stop_point = -1);
// post_api.hip
std::vector<double> gauss_table(const op_ctx* c);
int ensure_post(op_ctx* c, int n, int mh, int mw);
void post_shape(op_ctx* c, PostShape& s, int n, int lh, int lw, int mh, int mw, double img_len, double sx,
                double sy);
void optimal_size(int h, int w, int img_size, int stride, int* out_w, int* out_h);
int rerun_big_rec(op_ctx* c, const PostRecord& r, int f, const int32_t* d_cnt, PostBuffers** out);
int read_big(PostBuffers* B, double* poses, double* scores, int cap, op_frame_result* res);
void post_record(op_ctx* c, int kind, const MapSource* low, const float* full, int64_t fstride,
                 const PostShape& s);
int read_result(op_ctx* c, int frame, double* poses, double* scores, int cap, op_frame_result* res);
// staged.hip
int stage_maps_dev(op_ctx* c, const float* maps, int n, int lh, int lw, float** out);
int take_upload(op_ctx* c);
void staged_sizes(op_ctx* c, int* in_w, int* in_h, int* map_w, int* map_h);
int upload_one_frame(op_ctx* c, const uint8_t* bgr, int h, int w, int64_t row_stride);
// A new staged frame set, in two steps around whatever fills d_frames (op_stage_frames' copy,
// op_jpeg_stage's kernels): a pending op_upload_frames is replaced and d_frames holds `bytes`; then,
// the stream idle, the captured graph is dropped on a geometry change and the set is n frames of h x w
int stage_reserve(op_ctx* c, size_t bytes);
int stage_commit(op_ctx* c, int n, int h, int w);
// "no staged frames" (OP_ERR_STATE), or frames first .. first + n - 1 (n >= 1) outside them
int staged_range(op_ctx* c, const char* who, int32_t first, int32_t n);
#pragma GCC visibility pop

// Record an event pair around `fn`'s launches when profiling is on.
template <class Fn>
static int profiled(op_ctx* c, int cls, double flops, double bytes, Fn fn) {
  if (!c->prof || !((c->prof_mask >> cls) & 1)) return fn();
  if (c->prof_join && !c->pending.empty() && c->pending.back().cls == cls) {
    ProfPair& p = c->pending.back();  // the previous launch of this run ended with p.b: move p.b past fn
    const int rc = fn();
    OP_HIP_CHECK(hipEventRecord(p.b, c->stream));
    p.flops += flops;
    p.bytes += bytes;
    p.n += 1;
    return rc;
  }
  hipEvent_t a = pool_event(c), b = pool_event(c);
  if (!a || !b) return fn();
  OP_HIP_CHECK(hipEventRecord(a, c->stream));
  const int rc = fn();
  OP_HIP_CHECK(hipEventRecord(b, c->stream));
  c->pending.push_back(ProfPair{cls, a, b, flops, bytes, 1});
  return rc;
}

}  // namespace op
