// What the one-shot device calls share (labels, augment, masks, maskview, draw, overlay, body,
// keypoint: build tables on the host, allocate, upload, run one to three kernels, time them,
// download, free): the device selection, the scoped job that owns the buffers, the events and the first error, and the
// per-device "last device time" record.  Each unit keeps its own sequence of steps and its own
// kernel launches.  Nothing here is part of the library's interface.
#pragma once
#include <cstdint>
#include <mutex>
#include <vector>

#include "common.hpp"

namespace op {
#pragma GCC visibility push(hidden)

constexpr int kMaxDevices = 64;  // devices the one-shot calls and their *_last_ms records know

// Makes `device` current: OP_ERR_HIP when the runtime fails, "no HIP device N" outside the devices
// present (and kMaxDevices).
int use_device(const char* who, int device);

// The frame-batch arguments of op_draw and op_overlay: n frames of hw[2f] x hw[2f + 1] BGR pixels at
// bgr[f], row_stride[f] bytes per row, each with an image to write at out[f].
int check_frames(const char* who, int32_t n, const uint8_t* const* bgr, const int64_t* row_stride, const int32_t* hw,
                 uint8_t* const* out);

// One call's device work.  stream == nullptr: the null stream, blocking copies, hipDeviceSynchronize
// (the context-free calls); a context's stream: asynchronous copies behind whatever is queued there,
// hipStreamSynchronize.  The first failure sets "<who>: <what>: <HIP's words>" and OP_ERR_HIP, and
// every later step but the waiting does nothing.  Whatever the host hands to a step (and the job's
// buffers) must outlive what was queued: declare it before the job; finish() -- and, on a stream,
// the destructor when finish() was never reached -- waits before anything is freed.
class Job {
 public:
  Job(const char* who, hipStream_t stream) : who_(who), stream_(stream) {}
  Job(const Job&) = delete;
  Job& operator=(const Job&) = delete;
  ~Job();
  int status() const { return res_; }
  bool ok() const { return res_ == OP_OK; }
  hipStream_t stream() const { return stream_; }
  float ms() const { return ms_; }  // between begin() and end(), once finish() has succeeded
  void check(hipError_t e, const char* what);
  void* alloc(size_t bytes);  // null for zero bytes and after a failure
  void upload(void* dst, const void* src, size_t bytes, const char* what = "upload");
  void upload2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height,
                const char* what);
  void memset(void* dst, int value, size_t bytes);
  void download(void* dst, const void* src, size_t bytes, const char* what = "download");
  void begin();  // creates the two events and records the first
  void end();    // records the second
  int finish(const char* what);  // waits (on a stream: also after a failure), reads ms(); the status

 private:
  const char* who_;
  hipStream_t stream_;
  std::vector<void*> bufs_;
  hipEvent_t ev_[2] = {};
  int res_ = OP_OK;
  bool waited_ = false;
  float ms_ = 0.0f;
};

// The device time of a unit's last completed call, per device.  The unit that keeps more per call
// than the time (augment's path counters) writes it next to ms / ran under `mutex` itself.
struct LastMs {
  std::mutex mutex;
  double ms[kMaxDevices] = {};
  bool ran[kMaxDevices] = {};
  void done(int device, double v);
  // "bad device N" (OP_ERR_INVALID) or "no <what_ran> has completed on device N" (OP_ERR_STATE);
  // the caller holds `mutex`
  int check(const char* who, const char* what_ran, int device);
  int get(const char* who, const char* what_ran, int device, double* out);  // "null ms" first
};

#pragma GCC visibility pop
}  // namespace op
