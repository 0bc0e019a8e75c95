// Training-sample augmentation on the device (coco_data_loader.py:60-205, augment.py): the pixel
// path of a batch of host-drawn plans.  Every value is an integer, or an f32 produced by one
// explicitly rounded operation, in the order of augment.py's augment_np: the two agree bit for bit.
//
// Host (augment_pack, plain double / float operations, no contraction): the plans are validated;
// per sample the cv2.resize(INTER_LINEAR) axis coefficients (index, c0, c1) and, for the output
// rows and columns inside the crop window only, warpAffine's fixed-point terms (adelta, bdelta per
// column, X0, Y0 per row; AB_BITS = 10, 32 sub-pixel steps).  The remap weight tables (cubic 1024 x
// 16, linear 1024 x 4 shorts, every set summing to 1 << 15) and BGR2HSV's division tables are built
// once on the host and uploaded with every call; the kernels read them through the cache.
// Device, two kernels over the whole batch:
//   aug_resize: one thread per pixel of a sample's resized image, BGR and the 0/1 mask.
//   aug_fused: one workgroup per 16 x 16 tile of an output frame.  A pixel undoes the
//     flip, maps through the crop window to a rotated-image coordinate (outside: 127 / false), takes
//     its source coordinate from the axis terms, and the workgroup reduces the tile's source box
//     (LDS min / max).  A box of at most kBox x kBox pixels (any pure rotation's: 16 sqrt(2) + 4) is
//     staged in LDS once and the 16 cubic and 4 linear taps are read from there; a larger one (a
//     minifying matrix) reads global memory.  Then the colour distortion and the store, the three
//     channels of a pixel by one lane.  The rotated image is never written.
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "oneshot.hpp"

namespace op {
namespace {

constexpr int kTile = 16;
constexpr int kBox = 32;                 // LDS box side (pixels)
constexpr int kBoxPitch = kBox * 3 + 4;  // bytes per staged BGR row: 25 dwords, rows start one bank apart
constexpr int kMaskPitch = kBox + 4;
constexpr int kWarpBorder = 128;  // saturate_cast<uchar>(127.5)
constexpr int kCropPad = 127;     // (zeros + 127.5).astype('uint8')
constexpr int kMaxSide = 16384;

struct AugSample {
  int64_t src_off, msk_off;  // into the uploaded sources / masks (msk_off < 0: no mask)
  int64_t rs_off, rm_off;    // into the resized BGR / mask scratch
  int64_t src_stride;
  int32_t h, w, rw, rh;
  int32_t lin_off;   // into the int32 table buffer: [rw][3] then [rh][3]
  int32_t warp_off;  // [4][insize]: adelta, bdelta (by unflipped column), X0, Y0 (by row)
  int32_t x_from, y_from, x_to, y_to;  // window in the unflipped crop; x_to < x_from: empty
  int32_t colour, dh, ds, dv, flip;
};

struct AugArgs {
  const AugSample* samples;
  const int32_t* itab;     // per-sample axis tables, then sdiv[256], hdiv[256] at hsv_off
  const int16_t* cubic;    // [1024][16]
  const int16_t* linear;   // [1024][4]
  const uint8_t* src;
  const uint8_t* msk;
  uint8_t* rs;
  uint8_t* rm;
  uint8_t* out_bgr;
  uint8_t* out_mask;
  unsigned long long* counts;  // [2]: pixels warped from LDS, from global memory
  int32_t hsv_off, insize;
};

__device__ __forceinline__ int aug_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(256) void aug_resize(AugArgs a) {
  const AugSample s = a.samples[blockIdx.y];
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= s.rw * s.rh) return;
  const int dy = pix / s.rw, dx = pix % s.rw;
  const int32_t* tx = a.itab + s.lin_off + 3 * dx;
  const int32_t* ty = a.itab + s.lin_off + 3 * (s.rw + dy);
  const int x0 = tx[0], x1 = min(x0 + 1, s.w - 1), a0 = tx[1], a1 = tx[2];
  const int r0 = aug_clamp(ty[0], 0, s.h - 1), r1 = aug_clamp(ty[0] + 1, 0, s.h - 1), b0 = ty[1], b1 = ty[2];
  const uint8_t* p0 = a.src + s.src_off + (int64_t)r0 * s.src_stride;
  const uint8_t* p1 = a.src + s.src_off + (int64_t)r1 * s.src_stride;
  uint8_t* o = a.rs + s.rs_off + (int64_t)pix * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int h0 = (int)p0[x0 * 3 + c] * a0 + (int)p0[x1 * 3 + c] * a1;
    const int h1 = (int)p1[x0 * 3 + c] * a0 + (int)p1[x1 * 3 + c] * a1;
    o[c] = (uint8_t)aug_clamp(((((h0 >> 4) * b0) >> 16) + (((h1 >> 4) * b1) >> 16) + 2) >> 2, 0, 255);
  }
  int m = 0;
  if (s.msk_off >= 0) {  // resized as a 0/1 image, then != 0
    const uint8_t* m0 = a.msk + s.msk_off + (int64_t)r0 * s.w;
    const uint8_t* m1 = a.msk + s.msk_off + (int64_t)r1 * s.w;
    const int h0 = (int)(m0[x0] != 0) * a0 + (int)(m0[x1] != 0) * a1;
    const int h1 = (int)(m1[x0] != 0) * a0 + (int)(m1[x1] != 0) * a1;
    m = aug_clamp(((((h0 >> 4) * b0) >> 16) + (((h1 >> 4) * b1) >> 16) + 2) >> 2, 0, 255) != 0;
  }
  a.rm[s.rm_off + pix] = (uint8_t)m;
}

// cv2.cvtColor BGR2HSV (u8, H in 0..180), clip(channel + delta, 0, 255), HSV2BGR (f32 path)
__device__ __forceinline__ void aug_colour(const int32_t* __restrict__ sdiv, const int32_t* __restrict__ hdiv, int dh,
                                           int ds, int dv, int* px) {
  const int b = px[0], g = px[1], r = px[2];
  const int v = max(max(b, g), r), diff = v - min(min(b, g), r);
  int s = (diff * sdiv[v] + (1 << 11)) >> 12;
  int h = v == r ? g - b : (v == g ? b - r + 2 * diff : r - g + 4 * diff);
  h = (h * hdiv[diff] + (1 << 11)) >> 12;
  h += h < 0 ? 180 : 0;
  h = aug_clamp(aug_clamp(h, 0, 255) + dh, 0, 255);
  s = aug_clamp((s & 255) + ds, 0, 255);
  const int v8 = aug_clamp(v + dv, 0, 255);
  float fh = __fmul_rn((float)h, __fdiv_rn(6.0f, 180.0f));
  const float fs = __fmul_rn((float)s, __fdiv_rn(1.0f, 255.0f));
  const float fv = __fmul_rn((float)v8, __fdiv_rn(1.0f, 255.0f));
  float o[3];
  if (s == 0) {
    o[0] = o[1] = o[2] = fv;
  } else {
    while (fh >= 6.0f) fh = __fsub_rn(fh, 6.0f);
    const int sector = (int)floorf(fh);
    fh = __fsub_rn(fh, (float)sector);
    float tab[4];
    tab[0] = fv;
    tab[1] = __fmul_rn(fv, __fsub_rn(1.0f, fs));
    tab[2] = __fmul_rn(fv, __fsub_rn(1.0f, __fmul_rn(fs, fh)));
    tab[3] = __fmul_rn(fv, __fsub_rn(1.0f, __fmul_rn(fs, __fsub_rn(1.0f, fh))));
    // sector_data {1,3,0} {1,0,2} {3,0,1} {0,2,1} {0,1,3} {2,1,0}: two bits per entry, b | g << 2 | r << 4
    const unsigned codes[6] = {1u | 3u << 2 | 0u << 4, 1u | 0u << 2 | 2u << 4, 3u | 0u << 2 | 1u << 4,
                               0u | 2u << 2 | 1u << 4, 0u | 1u << 2 | 3u << 4, 2u | 1u << 2 | 0u << 4};
    const unsigned code = codes[sector];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const unsigned k = (code >> (2 * c)) & 3u;
      o[c] = k == 0 ? tab[0] : (k == 1 ? tab[1] : (k == 2 ? tab[2] : tab[3]));
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) px[c] = aug_clamp(__float2int_rn(__fmul_rn(o[c], 255.0f)), 0, 255);
}

// The 16 cubic taps of the image and the 4 linear taps of the mask around source pixel (sx, sy).
// img / msk hold the pixels [x0, x0 + bw) x [y0, y0 + bh) of the resized image with the given row
// pitches (the whole image, or the tile's staged box, which covers every in-image tap of the tile);
// taps outside the resized image (rw x rh) read the border.
__device__ __forceinline__ void aug_taps(const uint8_t* img, int pitch, const uint8_t* msk, int mpitch, int x0, int y0,
                                         int rw, int rh, int sx, int sy, const int16_t* wc, const int16_t* wl,
                                         bool has_mask, int* px, bool* mv) {
  int acc[3] = {0, 0, 0};
  int xo[4];
  bool xin[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x = sx - 1 + k;
    xin[k] = x >= 0 && x < rw;
    xo[k] = (x - x0) * 3;
  }
#pragma unroll
  for (int ky = 0; ky < 4; ++ky) {
    const int y = sy - 1 + ky;
    const bool yin = y >= 0 && y < rh;
    const uint8_t* row = img + (y - y0) * pitch;
#pragma unroll
    for (int kx = 0; kx < 4; ++kx) {
      const int wgt = wc[ky * 4 + kx];
      const bool in = yin && xin[kx];
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] += (in ? (int)row[xo[kx] + c] : kWarpBorder) * wgt;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) px[c] = aug_clamp((acc[c] + (1 << 14)) >> 15, 0, 255);
  int macc = 0;
  if (has_mask) {
#pragma unroll
    for (int ky = 0; ky < 2; ++ky)
#pragma unroll
      for (int kx = 0; kx < 2; ++kx) {
        const int x = sx + kx, y = sy + ky;
        const bool in = x >= 0 && x < rw && y >= 0 && y < rh;
        macc += (in ? (int)msk[(y - y0) * mpitch + (x - x0)] * 255 : 0) * (int)wl[ky * 2 + kx];
      }
  }
  *mv = aug_clamp((macc + (1 << 14)) >> 15, 0, 255) > 0;
}

__global__ __launch_bounds__(kTile* kTile) void aug_fused(AugArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t simg[kBox * kBoxPitch];
  __shared__ uint8_t smsk[kBox * kMaskPitch];
  __shared__ int sbox[4];  // min sx, max sx, min sy, max sy over the tile's window pixels
  const AugSample s = a.samples[blockIdx.z];
  const int tid = threadIdx.y * kTile + threadIdx.x;
  const int i = blockIdx.y * kTile + threadIdx.y, j = blockIdx.x * kTile + threadIdx.x;
  const bool active = i < a.insize && j < a.insize;
  const int jj = s.flip ? a.insize - 1 - j : j;  // the column before the flip
  const bool inwin = active && jj >= s.x_from && jj <= s.x_to && i >= s.y_from && i <= s.y_to;
  if (tid == 0) {
    sbox[0] = sbox[2] = INT_MAX;
    sbox[1] = sbox[3] = INT_MIN;
  }
  __syncthreads();
  int sx = 0, sy = 0, sel = 0;
  if (inwin) {
    const int32_t* wt = a.itab + s.warp_off;
    const int X = (int)((unsigned)wt[2 * a.insize + i] + (unsigned)wt[jj]) >> 5;  // int32 sums wrap
    const int Y = (int)((unsigned)wt[3 * a.insize + i] + (unsigned)wt[a.insize + jj]) >> 5;
    sx = aug_clamp(X >> 5, -32768, 32767);
    sy = aug_clamp(Y >> 5, -32768, 32767);
    sel = (Y & 31) * 32 + (X & 31);
    atomicMin(&sbox[0], sx);
    atomicMax(&sbox[1], sx);
    atomicMin(&sbox[2], sy);
    atomicMax(&sbox[3], sy);
  }
  __syncthreads();
  // the box of every tap of the tile (cubic: s-1 .. s+2), cut to the resized image; workgroup-uniform
  const bool any = sbox[0] <= sbox[1];
  const int bx0 = max(sbox[0] - 1, 0), bx1 = min(sbox[1] + 2, s.rw - 1);
  const int by0 = max(sbox[2] - 1, 0), by1 = min(sbox[3] + 2, s.rh - 1);
  const int bw = bx1 - bx0 + 1, bh = by1 - by0 + 1;  // <= 0: every tap is outside the image
  const bool staged = any && bw <= kBox && bh <= kBox;
  const uint8_t* rs = a.rs + s.rs_off;
  const uint8_t* rm = a.rm + s.rm_off;
  const bool has_mask = s.msk_off >= 0;
  if (staged && bw > 0 && bh > 0) {
    const int rowb = bw * 3;
    for (int k = tid; k < bh * rowb; k += kTile * kTile) {
      const int y = k / rowb, xb = k % rowb;
      simg[y * kBoxPitch + xb] = rs[((int64_t)(by0 + y) * s.rw + bx0) * 3 + xb];
    }
    if (has_mask)
      for (int k = tid; k < bh * bw; k += kTile * kTile) {
        const int y = k / bw, x = k % bw;
        smsk[y * kMaskPitch + x] = rm[(int64_t)(by0 + y) * s.rw + bx0 + x];
      }
  }
  __syncthreads();
  if (tid == 0 && any) {
    int cnt = 0;  // the window's pixels in this tile: a rectangle
    const int r0 = max((int)blockIdx.y * kTile, s.y_from), r1 = min((int)blockIdx.y * kTile + kTile - 1, min(s.y_to, a.insize - 1));
    for (int c = 0; c < kTile; ++c) {
      const int col = blockIdx.x * kTile + c;
      const int cc = s.flip ? a.insize - 1 - col : col;
      cnt += (col < a.insize && cc >= s.x_from && cc <= s.x_to) ? 1 : 0;
    }
    cnt *= max(r1 - r0 + 1, 0);
    atomicAdd(&a.counts[staged ? 0 : 1], (unsigned long long)cnt);
  }
  if (!active) return;
  int px[3] = {kCropPad, kCropPad, kCropPad};
  bool mv = false;
  if (inwin) {
    const int16_t* wl = a.linear + sel * 4;
    // one weight set: 32 bytes, two 16-byte loads; the 32 KiB table stays in global memory and the
    // cache serves it (copying it into LDS per workgroup measured slower: DESIGN §15)
    __attribute__((aligned(16))) int16_t wc[16];
    *(int4*)&wc[0] = *(const int4*)(a.cubic + sel * 16);
    *(int4*)&wc[8] = *(const int4*)(a.cubic + sel * 16 + 8);
    if (staged)
      aug_taps(simg, kBoxPitch, smsk, kMaskPitch, bx0, by0, s.rw, s.rh, sx, sy, wc, wl, has_mask, px, &mv);
    else
      aug_taps(rs, s.rw * 3, rm, s.rw, 0, 0, s.rw, s.rh, sx, sy, wc, wl, has_mask, px, &mv);
  }
  if (s.colour) aug_colour(a.itab + a.hsv_off, a.itab + a.hsv_off + 256, s.dh, s.ds, s.dv, px);
  const int64_t o = ((int64_t)blockIdx.z * a.insize + i) * a.insize + j;
  a.out_bgr[o * 3] = (uint8_t)px[0];
  a.out_bgr[o * 3 + 1] = (uint8_t)px[1];
  a.out_bgr[o * 3 + 2] = (uint8_t)px[2];
  a.out_mask[o] = mv ? 1 : 0;
}

// ---- host tables (float / double operations as augment.py states them) ----
struct AugTables {
  std::vector<int16_t> cubic, linear;
  int32_t sdiv[256], hdiv[256];
};

int sat_short(float v) {
  const float r = std::nearbyintf(v);
  return (int)(r < -32768.f ? -32768.f : (r > 32767.f ? 32767.f : r));
}

// initInterTab2D: set ay * 32 + ax = rows (y taps) of columns (x taps), corrected to sum to 1 << 15
// on the largest / smallest of the taps k/2, k/2 + 1 of each axis (augment.py _remap_table)
void remap_table(const float* tab1d, int k, std::vector<int16_t>* out) {
  out->assign((size_t)1024 * k * k, 0);
  const int c = k / 2, ce = c + 2 < k ? c + 2 : k;
  for (int ay = 0; ay < 32; ++ay)
    for (int ax = 0; ax < 32; ++ax) {
      int it[16], sum = 0;
      for (int ky = 0; ky < k; ++ky)
        for (int kx = 0; kx < k; ++kx) {
          const float v = tab1d[ay * k + ky] * tab1d[ax * k + kx];
          sum += it[ky * k + kx] = sat_short(v * 32768.0f);
        }
      const int diff = sum - 32768;
      if (diff != 0) {
        int mk = c * k + c, Mk = mk;
        for (int k1 = c; k1 < ce; ++k1)
          for (int k2 = c; k2 < ce; ++k2) {
            if (it[k1 * k + k2] < it[mk])
              mk = k1 * k + k2;
            else if (it[k1 * k + k2] > it[Mk])
              Mk = k1 * k + k2;
          }
        it[diff < 0 ? Mk : mk] -= diff;
      }
      for (int e = 0; e < k * k; ++e) (*out)[((size_t)ay * 32 + ax) * k * k + e] = (int16_t)it[e];
    }
}

const AugTables& aug_tables() {
  static const AugTables t = [] {
    AugTables t;
    float cub[32 * 4], lin[32 * 2];
    for (int i = 0; i < 32; ++i) {
      const float x = (float)i * (1.0f / 32.0f), A = -0.75f;  // interpolateCubic, cvcubic.hpp's operation order
      const float x1 = x + 1.0f, y = 1.0f - x;
      float* c = cub + 4 * i;
      c[0] = ((A * x1 - -3.75f) * x1 + -6.0f) * x1 - -3.0f;
      c[1] = ((1.25f * x - 2.25f) * x) * x + 1.0f;
      c[2] = ((1.25f * y - 2.25f) * y) * y + 1.0f;
      c[3] = ((1.0f - c[0]) - c[1]) - c[2];
      lin[2 * i] = 1.0f - x;
      lin[2 * i + 1] = x;
    }
    remap_table(cub, 4, &t.cubic);
    remap_table(lin, 2, &t.linear);
    t.sdiv[0] = t.hdiv[0] = 0;
    for (int v = 1; v < 256; ++v) {
      t.sdiv[v] = (int32_t)std::nearbyint((double)(255 << 12) / (double)v);
      t.hdiv[v] = (int32_t)std::nearbyint((double)(180 << 12) / (6.0 * (double)v));
    }
    return t;
  }();
  return t;
}

int64_t rint_i32(double v) {
  v = v < -2147483648.0 ? -2147483648.0 : (v > 2147483647.0 ? 2147483647.0 : v);
  return (int64_t)std::nearbyint(v);
}

// cv2.resize(INTER_LINEAR) axis coefficients (oracle/cvresize.py _coeffs): [dsize][3] = index, c0, c1
void linear_axis(int dsize, int ssize, bool clamp, std::vector<int32_t>* out) {
  const double scale = 1.0 / ((double)dsize / (double)ssize);
  for (int d = 0; d < dsize; ++d) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)std::floor(f);
    f = f - (float)s;
    if (clamp) {
      if (s < 0) {
        f = 0.0f;
        s = 0;
      }
      if (s >= ssize - 1) {
        f = 0.0f;
        s = ssize - 1;
      }
    }
    out->push_back(s);
    out->push_back(sat_short((1.0f - f) * 2048.0f));
    out->push_back(sat_short(f * 2048.0f));
  }
}

const char* const kAug = "op_augment";

struct AugHost {
  std::vector<AugSample> samples;
  std::vector<int32_t> itab;
  int64_t src_bytes = 0, msk_bytes = 0, rs_bytes = 0, rm_bytes = 0;
  int32_t hsv_off = 0, max_pix = 0;
};

int augment_pack(int32_t n, const uint8_t* const* bgr, const int64_t* row_stride, const uint8_t* const* mask,
                 const op_augment_plan* plans, int32_t insize, const uint8_t* out_bgr, const uint8_t* out_mask,
                 AugHost* out) {
  if (n < 1 || n > 65535) return invalid(kAug, "n must be in 1 .. 65535");
  if (insize < 1 || insize > kMaxSide) return invalid(kAug, "insize must be in 1 .. 16384");
  if (!bgr) return invalid(kAug, "null bgr array");
  if (!row_stride) return invalid(kAug, "null row_stride array");
  if (!plans) return invalid(kAug, "null plans array");
  if (!out_bgr) return invalid(kAug, "null out_bgr");
  if (!out_mask) return invalid(kAug, "null out_mask");
  for (int f = 0; f < n; ++f) {
    const op_augment_plan& p = plans[f];
    const std::string at = "plan " + std::to_string(f) + ": ";
    if (!bgr[f]) return invalid(kAug, at + "null bgr entry");
    if (p.insize != insize) return invalid(kAug, at + "insize differs from the call's");
    if (p.h < 1 || p.w < 1 || p.h > kMaxSide || p.w > kMaxSide) return invalid(kAug, at + "h, w must be in 1 .. 16384");
    if (row_stride[f] < (int64_t)p.w * 3) return invalid(kAug, at + "row_stride below 3 * w");
    if (p.rw < 1 || p.rh < 1 || p.rw > kMaxSide || p.rh > kMaxSide) return invalid(kAug, at + "rw, rh must be in 1 .. 16384");
    if (p.bw < 1 || p.bh < 1 || p.bw > kMaxSide || p.bh > kMaxSide) return invalid(kAug, at + "bw, bh must be in 1 .. 16384");
    for (int k = 0; k < 6; ++k)
      if (!std::isfinite(p.R[k])) return invalid(kAug, at + "non-finite matrix R");
    if ((int64_t)p.x2 - p.x1 != (int64_t)p.x_to - p.x_from || (int64_t)p.y2 - p.y1 != (int64_t)p.y_to - p.y_from)
      return invalid(kAug, at + "the copy window's two sides differ in size");
    const bool empty = p.x2 < p.x1 || p.y2 < p.y1;
    if (!empty && (p.x_from < 0 || p.x_to >= insize || p.y_from < 0 || p.y_to >= insize))
      return invalid(kAug, at + "the copy window does not fit insize");
    if (!empty && (p.x1 < 0 || p.x2 >= p.bw || p.y1 < 0 || p.y2 >= p.bh))
      return invalid(kAug, at + "the copy window does not fit the rotated size bw x bh");
    if (p.colour && (std::abs((int64_t)p.dh) > 10 || std::abs((int64_t)p.ds) > 40 || std::abs((int64_t)p.dv) > 30))
      return invalid(kAug, at + "colour deltas dh, ds, dv outside [-10, 10], [-40, 40], [-30, 30]");
  }
  out->samples.resize(n);
  for (int f = 0; f < n; ++f) {
    const op_augment_plan& p = plans[f];
    AugSample& s = out->samples[f];
    s.h = p.h;
    s.w = p.w;
    s.rw = p.rw;
    s.rh = p.rh;
    s.src_stride = (int64_t)p.w * 3;  // uploaded densely
    s.src_off = out->src_bytes;
    out->src_bytes += (int64_t)p.h * p.w * 3;
    s.msk_off = -1;
    if (mask && mask[f]) {
      s.msk_off = out->msk_bytes;
      out->msk_bytes += (int64_t)p.h * p.w;
    }
    s.rs_off = out->rs_bytes;
    out->rs_bytes += (int64_t)p.rw * p.rh * 3;
    s.rm_off = out->rm_bytes;
    out->rm_bytes += (int64_t)p.rw * p.rh;
    out->max_pix = std::max(out->max_pix, p.rw * p.rh);
    s.lin_off = (int32_t)out->itab.size();
    linear_axis(p.rw, p.w, true, &out->itab);
    linear_axis(p.rh, p.h, false, &out->itab);
    const bool empty = p.x2 < p.x1 || p.y2 < p.y1;
    s.x_from = empty ? 0 : p.x_from;
    s.x_to = empty ? -1 : p.x_to;
    s.y_from = empty ? 0 : p.y_from;
    s.y_to = empty ? -1 : p.y_to;
    s.colour = p.colour ? 1 : 0;
    s.dh = p.dh;
    s.ds = p.ds;
    s.dv = p.dv;
    s.flip = p.flip ? 1 : 0;
    // warpAffine: invert R as OpenCV does, then the fixed-point axis terms of the window's pixels
    double M[6];
    std::memcpy(M, p.R, sizeof(M));
    double D = M[0] * M[4] - M[1] * M[3];
    D = D != 0 ? 1.0 / D : 0.0;
    const double A11 = M[4] * D, A22 = M[0] * D;
    M[0] = A11;
    M[1] *= -D;
    M[3] *= -D;
    M[4] = A22;
    const double b1 = -M[0] * M[2] - M[1] * M[5], b2 = -M[3] * M[2] - M[4] * M[5];
    M[2] = b1;
    M[5] = b2;
    s.warp_off = (int32_t)out->itab.size();
    out->itab.resize(out->itab.size() + (size_t)4 * insize, 0);
    int32_t* wt = out->itab.data() + s.warp_off;
    for (int c = s.x_from; c <= s.x_to; ++c) {
      const double x = (double)(p.x1 + (c - p.x_from));
      wt[c] = (int32_t)rint_i32(M[0] * x * 1024.0);
      wt[insize + c] = (int32_t)rint_i32(M[3] * x * 1024.0);
    }
    for (int r = s.y_from; r <= s.y_to; ++r) {
      const double y = (double)(p.y1 + (r - p.y_from));
      wt[2 * insize + r] = (int32_t)(rint_i32((M[1] * y + M[2]) * 1024.0) + 16);
      wt[3 * insize + r] = (int32_t)(rint_i32((M[4] * y + M[5]) * 1024.0) + 16);
    }
    if (out->itab.size() > ((size_t)1 << 30)) return invalid(kAug, "tables too large");
  }
  const AugTables& t = aug_tables();
  out->hsv_off = (int32_t)out->itab.size();
  out->itab.insert(out->itab.end(), t.sdiv, t.sdiv + 256);
  out->itab.insert(out->itab.end(), t.hdiv, t.hdiv + 256);
  return OP_OK;
}

LastMs g_aug_last;
long long g_aug_counts[kMaxDevices][2];  // the LDS / fallback paths of the last call, under g_aug_last.mutex

}  // namespace
}  // namespace op

using namespace op;

extern "C" int op_augment_tables(int16_t* cubic, int16_t* linear, int32_t* sdiv, int32_t* hdiv) {
  const AugTables& t = aug_tables();
  if (cubic) std::memcpy(cubic, t.cubic.data(), t.cubic.size() * sizeof(int16_t));
  if (linear) std::memcpy(linear, t.linear.data(), t.linear.size() * sizeof(int16_t));
  if (sdiv) std::memcpy(sdiv, t.sdiv, sizeof(t.sdiv));
  if (hdiv) std::memcpy(hdiv, t.hdiv, sizeof(t.hdiv));
  return OP_OK;
}

extern "C" int op_augment(int32_t device, int32_t n, const uint8_t* const* bgr, const int64_t* row_stride,
                          const uint8_t* const* mask, const op_augment_plan* plans, int32_t insize, uint8_t* out_bgr,
                          uint8_t* out_mask) {
  AugHost ah;
  const int rc = augment_pack(n, bgr, row_stride, mask, plans, insize, out_bgr, out_mask, &ah);
  if (rc) return rc;
  const int rd = use_device(kAug, device);
  if (rd) return rd;
  const AugTables& t = aug_tables();
  const size_t plane = (size_t)insize * insize;
  const size_t cubic_bytes = t.cubic.size() * sizeof(int16_t), linear_bytes = t.linear.size() * sizeof(int16_t);
  unsigned long long counts[2] = {0, 0};
  Job job(kAug, nullptr);
  AugArgs a;
  a.samples = (const AugSample*)job.alloc(ah.samples.size() * sizeof(AugSample));
  a.itab = (const int32_t*)job.alloc(ah.itab.size() * sizeof(int32_t));
  a.cubic = (const int16_t*)job.alloc(cubic_bytes);
  a.linear = (const int16_t*)job.alloc(linear_bytes);
  uint8_t* src = (uint8_t*)job.alloc((size_t)ah.src_bytes);
  uint8_t* msk = (uint8_t*)job.alloc((size_t)ah.msk_bytes);
  a.src = src;
  a.msk = msk;
  a.rs = (uint8_t*)job.alloc((size_t)ah.rs_bytes);
  a.rm = (uint8_t*)job.alloc((size_t)ah.rm_bytes);
  a.out_bgr = (uint8_t*)job.alloc(n * plane * 3);
  a.out_mask = (uint8_t*)job.alloc(n * plane);
  a.counts = (unsigned long long*)job.alloc(sizeof(counts));
  a.hsv_off = ah.hsv_off;
  a.insize = insize;
  job.begin();
  job.upload((void*)a.samples, ah.samples.data(), ah.samples.size() * sizeof(AugSample), "samples upload");
  job.upload((void*)a.itab, ah.itab.data(), ah.itab.size() * sizeof(int32_t), "tables upload");
  job.upload((void*)a.cubic, t.cubic.data(), cubic_bytes, "cubic table upload");
  job.upload((void*)a.linear, t.linear.data(), linear_bytes, "linear table upload");
  job.memset(a.counts, 0, sizeof(counts));
  for (int f = 0; f < n && job.ok(); ++f) {
    const AugSample& s = ah.samples[f];
    job.upload2d(src + s.src_off, (size_t)s.w * 3, bgr[f], (size_t)row_stride[f], (size_t)s.w * 3, (size_t)s.h,
                 "image upload");
    if (s.msk_off >= 0) job.upload(msk + s.msk_off, mask[f], (size_t)s.h * s.w, "mask upload");
  }
  if (job.ok()) {
    hipLaunchKernelGGL(aug_resize, dim3((unsigned)((ah.max_pix + 255) / 256), (unsigned)n), dim3(256), 0, nullptr, a);
    job.check(hipGetLastError(), "aug_resize");
    const unsigned tiles = (unsigned)((insize + kTile - 1) / kTile);
    hipLaunchKernelGGL(aug_fused, dim3(tiles, tiles, (unsigned)n), dim3(kTile, kTile), 0, nullptr, a);
    job.check(hipGetLastError(), "aug_fused");
  }
  job.end();
  job.finish("kernels");
  job.download(counts, a.counts, sizeof(counts), "counts download");
  job.download(out_bgr, a.out_bgr, n * plane * 3, "image download");
  job.download(out_mask, a.out_mask, n * plane, "mask download");
  if (job.ok()) {
    std::lock_guard<std::mutex> lock(g_aug_last.mutex);
    g_aug_last.ms[device] = (double)job.ms();
    g_aug_last.ran[device] = true;
    g_aug_counts[device][0] = (long long)counts[0];
    g_aug_counts[device][1] = (long long)counts[1];
  }
  return job.status();
}

extern "C" int op_augment_last_ms(int32_t device, double* ms) {
  return g_aug_last.get("op_augment_last_ms", kAug, device, ms);
}

extern "C" int op_augment_last_paths(int32_t device, int64_t* counts) {
  const char* who = "op_augment_last_paths";
  if (!counts) return invalid(who, "null counts");
  std::lock_guard<std::mutex> lock(g_aug_last.mutex);
  const int rc = g_aug_last.check(who, kAug, device);
  if (rc) return rc;
  counts[0] = g_aug_counts[device][0];
  counts[1] = g_aug_counts[device][1];
  return OP_OK;
}
