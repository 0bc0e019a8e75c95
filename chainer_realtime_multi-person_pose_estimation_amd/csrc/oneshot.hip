// oneshot.hpp's definitions: no kernel, host code only.
#include "oneshot.hpp"

#include <string>

namespace op {

int use_device(const char* who, int device) {
  int ndev = 0;
  OP_HIP_CHECK(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev || device >= kMaxDevices) return invalid(who, "no HIP device " + std::to_string(device));
  OP_HIP_CHECK(hipSetDevice(device));
  return OP_OK;
}

int check_frames(const char* who, int32_t n, const uint8_t* const* bgr, const int64_t* row_stride, const int32_t* hw,
                 uint8_t* const* out) {
  if (!bgr) return invalid(who, "null bgr");
  if (!row_stride) return invalid(who, "null row_stride");
  if (!hw) return invalid(who, "null hw");
  if (!out) return invalid(who, "null out");
  for (int f = 0; f < n; ++f) {
    const std::string at = "frame " + std::to_string(f);
    if (hw[2 * f] < 1 || hw[2 * f] > 16384 || hw[2 * f + 1] < 1 || hw[2 * f + 1] > 16384)
      return invalid(who, "hw: " + at + ": h, w must be in 1 .. 16384");
    if (!bgr[f]) return invalid(who, "bgr: " + at + ": null image");
    if (!out[f]) return invalid(who, "out: " + at + ": null image");
    if (row_stride[f] < (int64_t)hw[2 * f + 1] * 3) return invalid(who, "row_stride: " + at + ": fewer than 3 w bytes per row");
  }
  return OP_OK;
}

void Job::check(hipError_t e, const char* what) {
  if (e == hipSuccess || res_) return;
  set_error(std::string(who_) + ": " + what + ": " + hipGetErrorString(e));
  res_ = OP_ERR_HIP;
}

void* Job::alloc(size_t bytes) {
  void* p = nullptr;
  if (res_ || !bytes) return p;
  check(hipMalloc(&p, bytes), "hipMalloc");
  if (res_) return nullptr;
  bufs_.push_back(p);
  return p;
}

void Job::upload(void* dst, const void* src, size_t bytes, const char* what) {
  if (res_ || !bytes) return;
  check(stream_ ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream_)
                : hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice),
        what);
}

void Job::upload2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height,
                   const char* what) {
  if (res_ || !width || !height) return;
  check(stream_ ? hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, hipMemcpyHostToDevice, stream_)
                : hipMemcpy2D(dst, dpitch, src, spitch, width, height, hipMemcpyHostToDevice),
        what);
}

void Job::memset(void* dst, int value, size_t bytes) {
  if (res_ || !bytes) return;
  check(stream_ ? hipMemsetAsync(dst, value, bytes, stream_) : hipMemset(dst, value, bytes), "hipMemset");
}

void Job::download(void* dst, const void* src, size_t bytes, const char* what) {
  if (res_ || !bytes) return;
  check(stream_ ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream_)
                : hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost),
        what);
}

void Job::begin() {
  for (int i = 0; i < 2 && !res_; ++i) check(hipEventCreate(&ev_[i]), "hipEventCreate");
  if (!res_) check(hipEventRecord(ev_[0], stream_), "hipEventRecord");
}

void Job::end() {
  if (!res_) check(hipEventRecord(ev_[1], stream_), "hipEventRecord");
}

int Job::finish(const char* what) {
  if (stream_)
    check(hipStreamSynchronize(stream_), what);
  else if (!res_)
    check(hipDeviceSynchronize(), what);
  waited_ = true;
  if (!res_ && ev_[1]) check(hipEventElapsedTime(&ms_, ev_[0], ev_[1]), "hipEventElapsedTime");
  return res_;
}

Job::~Job() {
  if (stream_ && !waited_) (void)hipStreamSynchronize(stream_);
  for (void* p : bufs_) (void)hipFree(p);
  for (hipEvent_t e : ev_)
    if (e) (void)hipEventDestroy(e);
}

void LastMs::done(int device, double v) {
  if (device < 0 || device >= kMaxDevices) return;
  std::lock_guard<std::mutex> lock(mutex);
  ms[device] = v;
  ran[device] = true;
}

int LastMs::check(const char* who, const char* what_ran, int device) {
  if (device < 0 || device >= kMaxDevices) return invalid(who, "bad device " + std::to_string(device));
  if (!ran[device]) {
    set_error(std::string(who) + ": no " + what_ran + " has completed on device " + std::to_string(device));
    return OP_ERR_STATE;
  }
  return OP_OK;
}

int LastMs::get(const char* who, const char* what_ran, int device, double* out) {
  if (!out) return invalid(who, "null ms");
  std::lock_guard<std::mutex> lock(mutex);
  const int rc = check(who, what_ran, device);
  if (!rc) *out = ms[device];
  return rc;
}

}  // namespace op
