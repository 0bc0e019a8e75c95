// Drives csrc/oneshot.hip's failure path on a machine without a HIP device, where every HIP call
// returns hipErrorNoDevice: one null-stream job through its whole step list, a LastMs record nobody
// completed and use_device.  Built with the host code under AddressSanitizer and run by
// tests/test_oneshot_host.py; exits 0 when every expectation holds (and ASan's leak check is clean).
#include <cstdio>
#include <string>
#include <vector>

#include "oneshot.hpp"

static std::string g_error;
static int g_errors_set = 0;
namespace op {
void set_error(const std::string& msg) {
  g_error = msg;
  ++g_errors_set;
}
}  // namespace op

static int g_failed = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("line %d: %s (last error: %s)\n", __LINE__, #cond, g_error.c_str()); \
      ++g_failed;                                                      \
    }                                                                  \
  } while (0)

int main() {
  const std::string none = hipGetErrorString(hipErrorNoDevice);
  EXPECT(none == "no ROCm-capable device is detected");
  {
    std::vector<char> host(64, 1), back(64, 2);
    op::Job job("op_test", nullptr);
    void* a = job.alloc(64);
    void* z = job.alloc(0);
    void* b = job.alloc(128);
    EXPECT(!a && !z && !b);
    EXPECT(job.status() == OP_ERR_HIP && !job.ok());
    EXPECT(g_error == "op_test: hipMalloc: " + none && g_errors_set == 1);
    job.begin();
    job.upload(a, host.data(), host.size());
    job.upload2d(b, 16, host.data(), 16, 16, 4, "frame upload");
    job.memset(b, 0, 128);
    job.end();
    EXPECT(job.finish("kernel") == OP_ERR_HIP);
    job.download(back.data(), a, back.size());
    EXPECT(job.status() == OP_ERR_HIP && job.ms() == 0.0f && back[0] == 2 && back[63] == 2);
    EXPECT(g_error == "op_test: hipMalloc: " + none && g_errors_set == 1);  // the first error won
  }
  {
    op::LastMs last;
    double ms = -1.0;
    EXPECT(last.get("op_test_last_ms", "op_test", 0, &ms) == OP_ERR_STATE && ms == -1.0);
    EXPECT(g_error == "op_test_last_ms: no op_test has completed on device 0");
    EXPECT(last.get("op_test_last_ms", "op_test", 0, nullptr) == OP_ERR_INVALID);
    EXPECT(last.get("op_test_last_ms", "op_test", op::kMaxDevices, &ms) == OP_ERR_INVALID);
    last.done(op::kMaxDevices, 1.0);  // out of range: ignored
    last.done(3, 0.25);
    EXPECT(last.get("op_test_last_ms", "op_test", 3, &ms) == OP_OK && ms == 0.25);
    EXPECT(last.get("op_test_last_ms", "op_test", 2, &ms) == OP_ERR_STATE);
  }
  EXPECT(op::use_device("x", 0) == OP_ERR_HIP);
  EXPECT(g_error == "hipGetDeviceCount(&ndev): " + none);
  if (!g_failed) std::printf("oneshot ok\n");
  return g_failed ? 1 : 0;
}
