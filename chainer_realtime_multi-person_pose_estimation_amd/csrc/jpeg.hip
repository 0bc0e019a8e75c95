// Baseline JPEG frames decoded on the device (jpeg.py's decode_np is the statement, and
// the two agree bit for bit).
//
// Host: jpeg_host.hpp parses the headers and entropy-decodes each file on a pool of threads into
// int16 coefficient blocks; jpeg_plan lays the batch out (a frame's blocks are contiguous: Y, Cb,
// Cr, each in raster order over its padded block grid) and writes one JpegFrame per decodable
// frame.  Two kernels cover the whole batch, whatever mix of sizes and samplings it holds
// (blockIdx.y = the frame, blockIdx.x runs over the largest frame's work):
//   jpeg_idct    8 lanes per 8x8 block, 32 blocks per 256-thread workgroup.  A lane loads one 16-byte
//                row, dequantises it, the block is transposed through LDS (8 x 9 dwords per block),
//                a lane runs jidctint's pass 1 down one column, the block is transposed back, a lane
//                runs pass 2 along one row and stores its 8 samples with one 8-byte store into the
//                component's plane (pitch = 8 x blocks per row).
//   jpeg_colour  a thread owns 4 consecutive pixels of the frame's dense BGR bytes, starting where
//                the destination is dword aligned: it reads the luma, computes the upsampled chroma
//                on the fly from the planes (libjpeg's fancy 2x1 / 2x2 filters, neighbours clamped at
//                the true plane edge, replication at chroma widths <= 2), converts, and stores three
//                dwords; the up to 3 pixels before the first aligned one and after the last whole
//                group are stored as bytes.
// The inverse DCT runs in 32-bit wrapping arithmetic (uint32_t): every value is then right modulo
// 2^32, and the eight sums a pass shifts down are exact whenever they fit int32, which
// sum |coef q| <= 32768 over the block guarantees (the host turns other frames down: OP_JPEG_RANGE).
#include <chrono>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "common.hpp"
#include "ctx.hpp"
#include "jpeg_host.hpp"
#include "oneshot.hpp"

namespace op {
namespace {

constexpr int kJpegThreads = 256;
constexpr int kIdctBlocks = kJpegThreads / 8;  // blocks per workgroup
constexpr int kTilePitch = 9;                  // dwords per row of a block in LDS
constexpr int kJpegMaxFrames = 65535;          // gridDim.y
constexpr int64_t kJpegMaxBlocks = (int64_t)1 << 25;  // 4 GiB of coefficients in one batch

struct JpegFrame {
  int64_t coef0;     // the frame's first block in the coefficient buffer
  int64_t plane[3];  // byte offsets of the component planes
  int64_t dst;       // byte offset of the frame's BGR pixels
  int32_t nb[3];     // blocks of each component (0: no such component)
  int32_t bw[3];     // blocks per row
  int32_t h, w, cw, ch;  // cw x ch: the true size of a chroma plane
  int32_t hs, vs, ncomp, box;  // box: chroma replicated, not filtered
  uint16_t q[3][64];
};
static_assert(sizeof(JpegFrame) % 16 == 0, "q rows are read 16 bytes at a time");

// jidctint's 8-point pass before the descale, modulo 2^32
__device__ __forceinline__ void idct_pass(const uint32_t* x, uint32_t* o) {
  uint32_t z1 = (x[2] + x[6]) * 4433u;
  const uint32_t t2 = z1 - x[6] * 15137u, t3 = z1 + x[2] * 6270u;
  const uint32_t t0 = (x[0] + x[4]) << 13, t1 = (x[0] - x[4]) << 13;
  const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  uint32_t a0 = x[7], a1 = x[5], a2 = x[3], a3 = x[1];
  z1 = a0 + a3;
  uint32_t z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
  const uint32_t z5 = (z3 + z4) * 9633u;
  a0 *= 2446u;
  a1 *= 16819u;
  a2 *= 25172u;
  a3 *= 12299u;
  z1 *= 0u - 7373u;
  z2 *= 0u - 20995u;
  z3 = z3 * (0u - 16069u) + z5;
  z4 = z4 * (0u - 3196u) + z5;
  a0 += z1 + z3;
  a1 += z2 + z4;
  a2 += z2 + z3;
  a3 += z1 + z4;
  o[0] = t10 + a3;
  o[1] = t11 + a2;
  o[2] = t12 + a1;
  o[3] = t13 + a0;
  o[4] = t13 - a0;
  o[5] = t12 - a1;
  o[6] = t11 - a2;
  o[7] = t10 - a3;
}

__device__ __forceinline__ int32_t descale(uint32_t v, int n) { return (int32_t)(v + (1u << (n - 1))) >> n; }

__global__ __launch_bounds__(kJpegThreads) void jpeg_idct(const JpegFrame* __restrict__ frames,
                                                          const int16_t* __restrict__ coef, uint8_t* __restrict__ planes) {
  __shared__ uint32_t tile[kIdctBlocks * 8 * kTilePitch];
  const JpegFrame& fr = frames[blockIdx.y];
  const int lane = threadIdx.x & 7, group = threadIdx.x >> 3;
  const int nb0 = fr.nb[0], nb1 = fr.nb[1], total = nb0 + nb1 + fr.nb[2];
  const int64_t b = (int64_t)blockIdx.x * kIdctBlocks + group;
  const bool live = b < total;
  int c = 0, bl = (int)(live ? b : 0);
  if (bl >= nb0) {
    bl -= nb0;
    c = 1;
    if (bl >= nb1) {
      bl -= nb1;
      c = 2;
    }
  }
  uint32_t x[8], o[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) x[k] = 0u;
  if (live) {
    const uint4 raw = *(const uint4*)(coef + (fr.coef0 + b) * 64 + lane * 8);
    const uint4 qr = *(const uint4*)(&fr.q[c][lane * 8]);
    const uint32_t rw[4] = {raw.x, raw.y, raw.z, raw.w}, qw[4] = {qr.x, qr.y, qr.z, qr.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      x[2 * k] = (uint32_t)((int32_t)(int16_t)(rw[k] & 0xffffu) * (int32_t)(qw[k] & 0xffffu));
      x[2 * k + 1] = (uint32_t)((int32_t)(int16_t)(rw[k] >> 16) * (int32_t)(qw[k] >> 16));
    }
  }
  uint32_t* t = tile + group * 8 * kTilePitch;
#pragma unroll
  for (int k = 0; k < 8; ++k) t[lane * kTilePitch + k] = x[k];  // row `lane`
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) x[k] = t[k * kTilePitch + lane];  // column `lane`
  idct_pass(x, o);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) t[k * kTilePitch + lane] = (uint32_t)descale(o[k], 11);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) x[k] = t[lane * kTilePitch + k];  // row `lane` of pass 1's output
  idct_pass(x, o);
  if (!live) return;
  uint32_t px[2] = {0u, 0u};
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    int32_t v = descale(o[k], 18) + 128;
    v = v < 0 ? 0 : (v > 255 ? 255 : v);
    px[k >> 2] |= (uint32_t)v << (8 * (k & 3));
  }
  const int bw = fr.bw[c], by = bl / bw, bx = bl - by * bw;
  uint8_t* p = planes + fr.plane[c] + ((int64_t)(by * 8 + lane) * bw + bx) * 8;
  *(uint2*)p = make_uint2(px[0], px[1]);
}

// The upsampled chroma sample at (y, x) of a plane of `pitch` bytes per row
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ pl, int pitch, int hs, int vs, int box, int cw, int ch,
                                         int y, int x) {
  if (hs == 1) return pl[(int64_t)y * pitch + x];
  const int cx = x >> 1, odd = x & 1;
  const int cxn = odd ? (cx + 1 < cw ? cx + 1 : cw - 1) : (cx > 0 ? cx - 1 : 0);
  if (vs == 1) {
    const uint8_t* r = pl + (int64_t)y * pitch;
    const int s = r[cx];
    return box ? s : (3 * s + r[cxn] + 1 + odd) >> 2;
  }
  const int cy = y >> 1;
  const uint8_t* r0 = pl + (int64_t)cy * pitch;
  if (box) return r0[cx];
  const int cyn = (y & 1) ? (cy + 1 < ch ? cy + 1 : ch - 1) : (cy > 0 ? cy - 1 : 0);
  const uint8_t* r1 = pl + (int64_t)cyn * pitch;
  const int v = 3 * r0[cx] + r1[cx], vn = 3 * r0[cxn] + r1[cxn];
  return (3 * v + vn + 8 - odd) >> 4;
}

__device__ __forceinline__ uint32_t clamp_u8(int v) { return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

__global__ __launch_bounds__(kJpegThreads) void jpeg_colour(const JpegFrame* __restrict__ frames,
                                                            const uint8_t* __restrict__ planes, uint8_t* __restrict__ out) {
  const JpegFrame& fr = frames[blockIdx.y];
  const int h = fr.h, w = fr.w, npix = h * w;  // at most 2^28
  uint8_t* dst = out + fr.dst;
  // pixel p begins at byte 3 p: the first dword-aligned pixel is pixel (address mod 4)
  const int head = (int)((uintptr_t)dst & 3u);
  const int64_t g = (int64_t)blockIdx.x * kJpegThreads + threadIdx.x;
  const int64_t start64 = 4 * g - ((4 - head) & 3);
  if (start64 >= npix) return;
  const int start = (int)start64;
  const int ncomp = fr.ncomp, hs = fr.hs, vs = fr.vs, box = fr.box, cw = fr.cw, ch = fr.ch;
  const uint8_t* py = planes + fr.plane[0];
  const uint8_t* pb = planes + fr.plane[1];
  const uint8_t* pr = planes + fr.plane[2];
  const int ypitch = fr.bw[0] * 8, cpitch = fr.bw[1] * 8;
  const int first = start < 0 ? 0 : start;
  int y = first / w, x = first - y * w;
  uint32_t px[4] = {0u, 0u, 0u, 0u};  // B | G << 8 | R << 16
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int p = start + k;
    if (p < 0 || p >= npix) continue;
    const int lum = py[(int64_t)y * ypitch + x];
    if (ncomp == 1) {
      px[k] = (uint32_t)lum * 0x010101u;
    } else {
      const int cb = chroma_at(pb, cpitch, hs, vs, box, cw, ch, y, x) - 128;
      const int cr = chroma_at(pr, cpitch, hs, vs, box, cw, ch, y, x) - 128;
      const int r = lum + ((91881 * cr + 32768) >> 16);
      const int b = lum + ((116130 * cb + 32768) >> 16);
      const int gq = lum + ((-22554 * cb - 46802 * cr + 32768) >> 16);
      px[k] = clamp_u8(b) | (clamp_u8(gq) << 8) | (clamp_u8(r) << 16);
    }
    if (++x == w) {
      x = 0;
      ++y;
    }
  }
  if (start >= 0 && start + 3 < npix) {
    uint32_t* d = (uint32_t*)(dst + (int64_t)3 * start);
    d[0] = px[0] | (px[1] << 24);
    d[1] = (px[1] >> 8) | (px[2] << 16);
    d[2] = (px[2] >> 16) | (px[3] << 8);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int p = start + k;
      if (p < 0 || p >= npix) continue;
      uint8_t* d = dst + (int64_t)3 * p;
      d[0] = (uint8_t)(px[k] & 255u);
      d[1] = (uint8_t)((px[k] >> 8) & 255u);
      d[2] = (uint8_t)((px[k] >> 16) & 255u);
    }
  }
}

// ---- host ----
struct JpegGeo {
  int32_t status = jpeg::kOk;
  int32_t h = 0, w = 0;
  int64_t blocks = 0, coef0 = 0;
  JpegFrame fr;
};

struct JpegPlan {
  std::vector<JpegGeo> geo;  // per frame of the call
  int64_t blocks = 0, plane_bytes = 0;
  unsigned idct_groups = 0, colour_groups = 0;  // gridDim.x: the largest frame's
};

// Parses frame f's header and lays its blocks and planes out behind the frames before it
void jpeg_plan_frame(JpegPlan* plan, int f, const uint8_t* data, size_t bytes, int want_h, int want_w) {
  JpegGeo& g = plan->geo[f];
  jpeg::Header hd;
  g.status = jpeg::parse_header(data, bytes, &hd);
  if (g.status != jpeg::kOk) return;
  g.h = hd.h;
  g.w = hd.w;
  if (want_h && (hd.h != want_h || hd.w != want_w)) {
    g.status = jpeg::kSize;
    return;
  }
  JpegFrame& fr = g.fr;
  memset(&fr, 0, sizeof(fr));
  g.blocks = hd.blocks;
  g.coef0 = fr.coef0 = plan->blocks;
  plan->blocks += hd.blocks;
  for (int c = 0; c < hd.ncomp; ++c) {
    fr.nb[c] = hd.bw[c] * hd.bh[c];
    fr.bw[c] = hd.bw[c];
    fr.plane[c] = plan->plane_bytes;
    plan->plane_bytes += (int64_t)fr.nb[c] * 64;  // a multiple of 64: every plane stays 8-byte aligned
    memcpy(fr.q[c], hd.qt[hd.tq[c]], 128);
  }
  fr.h = hd.h;
  fr.w = hd.w;
  fr.hs = hd.hs;
  fr.vs = hd.vs;
  fr.ncomp = hd.ncomp;
  fr.cw = (hd.w + hd.hs - 1) / hd.hs;
  fr.ch = (hd.h + hd.vs - 1) / hd.vs;
  fr.box = fr.cw <= 2;
}

// The descriptors of the frames that decoded (status kOk), dst set by the caller's rule; sizes the grids
template <class Dst>
int jpeg_live(JpegPlan* plan, JpegFrame* out, Dst dst) {
  int live = 0;
  plan->idct_groups = plan->colour_groups = 0;
  for (size_t f = 0; f < plan->geo.size(); ++f) {
    JpegGeo& g = plan->geo[f];
    if (g.status != jpeg::kOk || !g.blocks) continue;
    g.fr.dst = dst((int)f);
    out[live++] = g.fr;
    const unsigned ig = (unsigned)((g.blocks + kIdctBlocks - 1) / kIdctBlocks);
    // a group of 4 pixels per thread, and one more for the pixels before the first aligned one
    const unsigned cg = (unsigned)(((int64_t)g.h * g.w / 4 + 2 + kJpegThreads - 1) / kJpegThreads);
    plan->idct_groups = ig > plan->idct_groups ? ig : plan->idct_groups;
    plan->colour_groups = cg > plan->colour_groups ? cg : plan->colour_groups;
  }
  return live;
}

void jpeg_launch(Job& job, const JpegPlan& plan, int live, const JpegFrame* d_frames, const int16_t* d_coef,
                 uint8_t* d_planes, uint8_t* d_out) {
  if (!job.ok() || !live) return;
  hipLaunchKernelGGL(jpeg_idct, dim3(plan.idct_groups, (unsigned)live), dim3(kJpegThreads), 0, job.stream(), d_frames,
                     d_coef, d_planes);
  job.check(hipGetLastError(), "jpeg_idct");
  hipLaunchKernelGGL(jpeg_colour, dim3(plan.colour_groups, (unsigned)live), dim3(kJpegThreads), 0, job.stream(), d_frames,
                     d_planes, d_out);
  job.check(hipGetLastError(), "jpeg_colour");
}

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// host entropy-decode wall time and device time of the last completed call, per device
struct JpegLast {
  LastMs dev;
  double host[kMaxDevices] = {};
  void done(int device, double host_ms, double dev_ms) {
    if (device < 0 || device >= kMaxDevices) return;
    std::lock_guard<std::mutex> lock(dev.mutex);
    dev.ms[device] = dev_ms;
    dev.ran[device] = true;
    host[device] = host_ms;
  }
} g_jpeg_last;

int check_files(const char* who, int f, const uint8_t* data, int64_t bytes) {
  const std::string at = "frame " + std::to_string(f);
  if (!data) return invalid(who, "data: " + at + ": null file");
  if (bytes < 0) return invalid(who, "bytes: " + at + ": negative");
  return OP_OK;
}

}  // namespace
}  // namespace op

using namespace op;

extern "C" int op_jpeg_probe(const uint8_t* data, int64_t bytes, op_jpeg_info* out) {
  const char* who = "op_jpeg_probe";
  if (!data) return invalid(who, "null data");
  if (bytes < 0) return invalid(who, "negative bytes");
  if (!out) return invalid(who, "null out");
  memset(out, 0, sizeof(*out));
  jpeg::Header hd;
  out->status = jpeg::parse_header(data, (size_t)bytes, &hd);
  if (out->status != jpeg::kOk) return OP_OK;
  out->h = hd.h;
  out->w = hd.w;
  out->components = hd.ncomp;
  out->hs = hd.hs;
  out->vs = hd.vs;
  for (int c = 0; c < hd.ncomp; ++c) {
    out->blocks_w[c] = hd.bw[c];
    out->blocks_h[c] = hd.bh[c];
  }
  out->n_blocks = hd.blocks;
  return OP_OK;
}

extern "C" int op_jpeg_coefficients(const uint8_t* data, int64_t bytes, int16_t* coef, int64_t coef_cap, uint16_t* qt,
                                    int32_t* status) {
  const char* who = "op_jpeg_coefficients";
  if (!data) return invalid(who, "null data");
  if (bytes < 0) return invalid(who, "negative bytes");
  if (!coef) return invalid(who, "null coef");
  if (!qt) return invalid(who, "null qt");
  if (!status) return invalid(who, "null status");
  jpeg::Header hd;
  *status = jpeg::parse_header(data, (size_t)bytes, &hd);
  if (*status != jpeg::kOk) return OP_OK;
  if (coef_cap < hd.blocks * 64)
    return invalid(who, "coef_cap: " + std::to_string(hd.blocks * 64) + " coefficients are needed");
  for (int c = 0; c < hd.ncomp; ++c) memcpy(qt + 64 * c, hd.qt[hd.tq[c]], 128);
  *status = jpeg::decode_scan(data, (size_t)bytes, hd, coef);
  return OP_OK;
}

extern "C" int op_jpeg_block_in_range(const int16_t* coef, const uint16_t* q, int32_t* in_range) {
  const char* who = "op_jpeg_block_in_range";
  if (!coef || !q || !in_range) return invalid(who, "null argument");
  *in_range = jpeg::block_in_range(coef, q) ? 1 : 0;
  return OP_OK;
}

extern "C" int op_jpeg_set_threads(int32_t threads) {
  if (threads < 0 || threads > 64) return invalid("op_jpeg_set_threads", "threads must be in 1 .. 64, or 0 for the default");
  jpeg::pool_threads().store(threads);
  return OP_OK;
}

extern "C" int op_jpeg_last_ms(int32_t device, double* ms) {
  const char* who = "op_jpeg_last_ms";
  if (!ms) return invalid(who, "null ms");
  std::lock_guard<std::mutex> lock(g_jpeg_last.dev.mutex);
  RC(g_jpeg_last.dev.check(who, "op_jpeg_decode or op_jpeg_stage", device));
  ms[0] = g_jpeg_last.host[device];
  ms[1] = g_jpeg_last.dev.ms[device];
  return OP_OK;
}

namespace op {
namespace {

int jpeg_decode(const char* who, int32_t device, int32_t n, const uint8_t* const* data, const int64_t* bytes,
                uint8_t* const* out, int32_t* status) {
  if (n < 0 || n > kJpegMaxFrames) return invalid(who, "n must be in 0 .. 65535");
  if (n == 0) return OP_OK;
  if (!data) return invalid(who, "null data");
  if (!bytes) return invalid(who, "null bytes");
  if (!out) return invalid(who, "null out");
  if (!status) return invalid(who, "null status");
  for (int f = 0; f < n; ++f) RC(check_files(who, f, data[f], bytes[f]));
  JpegPlan plan;
  plan.geo.resize((size_t)n);
  std::vector<int64_t> dst((size_t)n + 1, 0);
  for (int f = 0; f < n; ++f) {
    jpeg_plan_frame(&plan, f, data[f], (size_t)bytes[f], 0, 0);
    const JpegGeo& g = plan.geo[f];
    if (g.status == jpeg::kOk && !out[f]) return invalid(who, "out: frame " + std::to_string(f) + ": null image");
    dst[f + 1] = dst[f] + (g.status == jpeg::kOk ? pad16((int64_t)g.h * g.w * 3) : 0);
    if (plan.blocks > kJpegMaxBlocks) return invalid(who, "more than 2^25 coefficient blocks in the batch");
  }
  std::vector<int16_t> coef((size_t)plan.blocks * 64);
  std::vector<jpeg::Task> tasks((size_t)n);
  for (int f = 0; f < n; ++f)
    tasks[f] = jpeg::Task{data[f], (size_t)bytes[f], coef.data() + plan.geo[f].coef0 * 64, plan.geo[f].status};
  const auto t0 = std::chrono::steady_clock::now();
  jpeg::decode_batch(tasks.data(), n);
  const double host_ms = ms_since(t0);
  for (int f = 0; f < n; ++f) status[f] = plan.geo[f].status = tasks[f].status;
  std::vector<JpegFrame> frames((size_t)n);
  const int live = jpeg_live(&plan, frames.data(), [&](int f) { return dst[f]; });
  if (!live) return OP_OK;  // no device call: nothing completed on `device`, nothing is recorded
  RC(use_device(who, device));
  Job job(who, nullptr);
  JpegFrame* d_frames = (JpegFrame*)job.alloc((size_t)live * sizeof(JpegFrame));
  int16_t* d_coef = (int16_t*)job.alloc(coef.size() * 2);
  uint8_t* d_planes = (uint8_t*)job.alloc((size_t)plan.plane_bytes);
  uint8_t* d_out = (uint8_t*)job.alloc((size_t)dst[n]);
  job.begin();
  job.upload(d_frames, frames.data(), (size_t)live * sizeof(JpegFrame), "table upload");
  job.upload(d_coef, coef.data(), coef.size() * 2, "coefficient upload");
  jpeg_launch(job, plan, live, d_frames, d_coef, d_planes, d_out);
  job.end();
  job.finish("kernel");
  for (int f = 0; f < n; ++f)
    if (status[f] == jpeg::kOk) job.download(out[f], d_out + dst[f], (size_t)plan.geo[f].h * plan.geo[f].w * 3);
  if (job.ok()) g_jpeg_last.done(device, host_ms, job.ms());
  return job.status();
}

int jpeg_stage(const char* who, op_ctx* c, int32_t n, const uint8_t* const* data, const int64_t* bytes,
               const uint8_t* const* bgr, int32_t h, int32_t w, int32_t* status) {
  if (!c) return invalid(who, "null context");
  if (n < 1 || n > kJpegMaxFrames) return invalid(who, "n must be in 1 .. 65535");
  if (h < 8 || w < 8 || h > jpeg::kMaxSide || w > jpeg::kMaxSide) return invalid(who, "h, w must be in 8 .. 16384");
  if (!status) return invalid(who, "null status");
  if (!bgr && (!data || !bytes)) return invalid(who, "null data or bytes without bgr");
  int given = 0;
  for (int f = 0; f < n; ++f) {
    if (bgr && bgr[f]) {
      ++given;
      continue;
    }
    if (!data || !bytes) return invalid(who, "frame " + std::to_string(f) + ": neither pixels nor a file");
    RC(check_files(who, f, data[f], bytes[f]));
  }
  RC(check_ctx(c, false));
  const size_t fbytes = (size_t)h * w * 3;
  JpegPlan plan;
  plan.geo.resize((size_t)n);
  for (int f = 0; f < n; ++f) {
    if (bgr && bgr[f]) continue;  // blocks 0: no part in the decode
    jpeg_plan_frame(&plan, f, data[f], (size_t)bytes[f], h, w);
    if (plan.blocks > kJpegMaxBlocks) return invalid(who, "more than 2^25 coefficient blocks in the batch");
  }
  // page-locked staging, one buffer: [descriptors | coefficients | the frames given as pixels]; the
  // first two go up in one copy
  const size_t tab_bytes = (size_t)n * sizeof(JpegFrame), coef_bytes = (size_t)plan.blocks * 128;
  const size_t up_bytes = tab_bytes + coef_bytes, pin_bytes = up_bytes + (size_t)given * fbytes;
  OP_HIP_CHECK(hipStreamSynchronize(c->stream));  // the staging buffer's previous copies have completed
  if (pin_bytes > c->jpeg_pinned_bytes) {
    if (c->jpeg_pinned) OP_HIP_CHECK(hipHostFree(c->jpeg_pinned));
    c->jpeg_pinned = nullptr;
    c->jpeg_pinned_bytes = 0;
    OP_HIP_CHECK(hipHostMalloc((void**)&c->jpeg_pinned, pin_bytes, hipHostMallocDefault));
    c->jpeg_pinned_bytes = pin_bytes;
  }
  RC(grow_buffer(c, (void**)&c->d_jpeg, &c->jpeg_bytes, up_bytes + (size_t)plan.plane_bytes, "jpeg"));
  RC(stage_reserve(c, fbytes * n));
  int16_t* coef = (int16_t*)(c->jpeg_pinned + tab_bytes);
  std::vector<jpeg::Task> tasks((size_t)n);
  for (int f = 0; f < n; ++f) {
    const bool file = !(bgr && bgr[f]);
    tasks[f] = jpeg::Task{file ? data[f] : nullptr, file ? (size_t)bytes[f] : 0, coef + plan.geo[f].coef0 * 64,
                          file ? plan.geo[f].status : -1};
  }
  const auto t0 = std::chrono::steady_clock::now();
  jpeg::decode_batch(tasks.data(), n);
  const double host_ms = ms_since(t0);
  for (int f = 0; f < n; ++f) {
    if (tasks[f].status >= 0) plan.geo[f].status = tasks[f].status;
    status[f] = plan.geo[f].status;  // a frame given as pixels: kOk
  }
  const int live = jpeg_live(&plan, (JpegFrame*)c->jpeg_pinned, [&](int f) { return (int64_t)((size_t)f * fbytes); });
  uint8_t* pix = c->jpeg_pinned + up_bytes;
  for (int f = 0, k = 0; f < n; ++f)
    if (bgr && bgr[f]) memcpy(pix + (size_t)k++ * fbytes, bgr[f], fbytes);
  Job job(who, c->stream);  // everything is ordered on the context stream
  job.begin();
  if (live) job.upload(c->d_jpeg, c->jpeg_pinned, up_bytes, "coefficient upload");
  for (int f = 0, k = 0; f < n; ++f) {
    if (bgr && bgr[f])
      job.upload(c->d_frames + (size_t)f * fbytes, pix + (size_t)k++ * fbytes, fbytes, "frame upload");
    else if (status[f] != jpeg::kOk)
      job.memset(c->d_frames + (size_t)f * fbytes, 0, fbytes);
  }
  jpeg_launch(job, plan, live, (const JpegFrame*)c->d_jpeg, (const int16_t*)(c->d_jpeg + tab_bytes), c->d_jpeg + up_bytes,
              c->d_frames);
  job.end();
  if (job.finish("kernel") != OP_OK) return job.status();
  RC(stage_commit(c, n, h, w));
  g_jpeg_last.done(c->device, host_ms, job.ms());
  return OP_OK;
}

// The host tables of a batch are sized by the files' headers (at most kJpegMaxBlocks blocks): an
// allocation that fails comes back as a status, not as an exception through the C interface
int out_of_memory(const char* who) {
  set_error(std::string(who) + ": out of host memory for the batch's tables");
  return OP_ERR_CAPACITY;
}

}  // namespace
}  // namespace op

extern "C" int op_jpeg_decode(int32_t device, int32_t n, const uint8_t* const* data, const int64_t* bytes,
                              uint8_t* const* out, int32_t* status) {
  try {
    return jpeg_decode("op_jpeg_decode", device, n, data, bytes, out, status);
  } catch (const std::bad_alloc&) {
    return out_of_memory("op_jpeg_decode");
  }
}

extern "C" int op_jpeg_stage(op_ctx* c, int32_t n, const uint8_t* const* data, const int64_t* bytes,
                             const uint8_t* const* bgr, int32_t h, int32_t w, int32_t* status) {
  try {
    return jpeg_stage("op_jpeg_stage", c, n, data, bytes, bgr, h, w, status);
  } catch (const std::bad_alloc&) {
    return out_of_memory("op_jpeg_stage");
  }
}
