// The host half of the JPEG decode: header parse and Huffman entropy decode of one
// baseline file into quantised coefficient blocks, exactly the layout jpeg.py's coefficients_np
// states, and the thread pool that runs a batch of them.  Plain C++17: no HIP, no exceptions, no
// allocation sized by the file (the caller sizes the coefficient storage from the parsed header,
// whose h and w are within 1 .. 16384 and whose block count the scan's length bounds), every read
// checked against the end of the data.
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

namespace op {
namespace jpeg {

constexpr int kOk = 0, kUnsupported = 1, kCorrupt = 2, kSize = 3, kRange = 4;  // OP_JPEG_*
constexpr int kMaxSide = 16384;
// sum over a block of |coef[k] * q[k]| up to which the kernel's 32-bit inverse DCT is exact
constexpr int64_t kRangeSum = 32768;
constexpr int kLook = 9;  // bits of the Huffman lookahead table

static const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Huff {
  bool present = false;
  uint8_t look_len[1 << kLook];  // code length of the code the next kLook bits begin with, 0: longer
  uint8_t look_sym[1 << kLook];
  int32_t maxcode[18];  // largest code of each length, -1 without one; [17] ends every search
  int32_t valoff[17];   // symbol index of a code = code + valoff[length]
  uint8_t sym[256];
};

struct Header {
  int32_t h = 0, w = 0, ncomp = 0, hs = 0, vs = 0;  // hs x vs: the luma's sampling (chroma 1 x 1)
  int32_t bw[3] = {0, 0, 0}, bh[3] = {0, 0, 0};     // padded block grid of each component
  int32_t tq[3] = {0, 0, 0}, td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
  int32_t ids[3] = {0, 0, 0};
  int32_t ri = 0;
  bool have_qt[4] = {false, false, false, false};
  uint16_t qt[4][64];  // natural order
  Huff huff[2][4];
  size_t scan = 0;  // where the entropy-coded data begin
  int64_t blocks = 0;
};

// T.81 Annex C: the decoding tables of one DHT entry; false when the lengths overflow a prefix code
inline bool build_huff(const uint8_t* counts, const uint8_t* symbols, int total, Huff* t) {
  memset(t->look_len, 0, sizeof(t->look_len));
  memset(t->look_sym, 0, sizeof(t->look_sym));
  memcpy(t->sym, symbols, (size_t)total);
  int32_t code = 0, k = 0;
  for (int len = 1; len <= 16; ++len) {
    t->valoff[len] = k - code;
    for (int i = 0; i < counts[len - 1]; ++i, ++code, ++k) {
      if (code >= (1 << len)) return false;
      if (len <= kLook) {
        const int lo = code << (kLook - len);
        for (int j = 0; j < (1 << (kLook - len)); ++j) {
          t->look_len[lo + j] = (uint8_t)len;
          t->look_sym[lo + j] = symbols[k];
        }
      }
    }
    t->maxcode[len] = counts[len - 1] ? code - 1 : -1;
    code <<= 1;
  }
  t->maxcode[17] = 0x7fffffff;
  t->present = true;
  return true;
}

// The segments up to and including the SOS header -> kOk and *hd, or the status
inline int parse_header(const uint8_t* d, size_t n, Header* hd) {
  if (!d || n < 4 || d[0] != 0xFF || d[1] != 0xD8) return kCorrupt;
  bool have_sof = false;
  size_t p = 2;
  for (;;) {
    if (p >= n || d[p] != 0xFF) return kCorrupt;
    while (p < n && d[p] == 0xFF) ++p;  // fill bytes
    if (p >= n) return kCorrupt;
    const int m = d[p++];
    if ((m >= 0xC1 && m <= 0xCF && m != 0xC4) || m == 0xDC || m == 0xDE || m == 0xDF || (m >= 0xF0 && m <= 0xFD))
      return kUnsupported;
    if (m < 0xC0 || (m >= 0xD0 && m <= 0xD9)) return kCorrupt;
    if (p + 2 > n) return kCorrupt;
    const size_t ln = ((size_t)d[p] << 8) | d[p + 1];
    if (ln < 2 || p + ln > n) return kCorrupt;
    const uint8_t* seg = d + p + 2;
    const size_t sl = ln - 2;
    p += ln;
    if (m == 0xC0) {
      if (have_sof || sl < 6) return kCorrupt;
      const int prec = seg[0], h = (seg[1] << 8) | seg[2], w = (seg[3] << 8) | seg[4], nc = seg[5];
      if (sl != 6 + 3 * (size_t)nc || w == 0 || nc == 0) return kCorrupt;
      if (prec != 8 || h == 0 || (nc != 1 && nc != 3) || h > kMaxSide || w > kMaxSide) return kUnsupported;
      int sh[3], sv[3];
      for (int i = 0; i < nc; ++i) {
        hd->ids[i] = seg[6 + 3 * i];
        sh[i] = seg[7 + 3 * i] >> 4;
        sv[i] = seg[7 + 3 * i] & 15;
        hd->tq[i] = seg[8 + 3 * i];
      }
      for (int i = 0; i < nc; ++i)
        if (sh[i] < 1 || sh[i] > 4 || sv[i] < 1 || sv[i] > 4 || hd->tq[i] > 3) return kCorrupt;
      for (int i = 0; i < nc; ++i)
        for (int j = 0; j < i; ++j)
          if (hd->ids[i] == hd->ids[j]) return kCorrupt;
      if (nc == 1) {
        if (sh[0] != 1 || sv[0] != 1) return kUnsupported;
      } else {
        const bool luma = (sh[0] == 1 && sv[0] == 1) || (sh[0] == 2 && sv[0] == 1) || (sh[0] == 2 && sv[0] == 2);
        if (!luma || sh[1] != 1 || sv[1] != 1 || sh[2] != 1 || sv[2] != 1) return kUnsupported;
        if (hd->ids[0] == 82 && hd->ids[1] == 71 && hd->ids[2] == 66) return kUnsupported;  // "RGB"
      }
      hd->h = h;
      hd->w = w;
      hd->ncomp = nc;
      hd->hs = sh[0];
      hd->vs = sv[0];
      have_sof = true;
    } else if (m == 0xC4) {
      size_t q = 0;
      while (q < sl) {
        if (q + 17 > sl) return kCorrupt;
        const int tc = seg[q] >> 4, th = seg[q] & 15;
        int total = 0;
        for (int i = 0; i < 16; ++i) total += seg[q + 1 + i];
        if (tc > 1 || th > 3 || total > 256 || q + 17 + (size_t)total > sl) return kCorrupt;
        if (tc == 0)
          for (int i = 0; i < total; ++i)
            if (seg[q + 17 + i] > 15) return kCorrupt;
        if (!build_huff(seg + q + 1, seg + q + 17, total, &hd->huff[tc][th])) return kCorrupt;
        q += 17 + (size_t)total;
      }
    } else if (m == 0xDB) {
      size_t q = 0;
      while (q < sl) {
        const int pq = seg[q] >> 4, tq = seg[q] & 15;
        if (pq > 1 || tq > 3) return kCorrupt;
        if (pq == 1) return kUnsupported;
        if (q + 65 > sl) return kCorrupt;
        for (int k = 0; k < 64; ++k) hd->qt[tq][kZigzag[k]] = seg[q + 1 + k];
        hd->have_qt[tq] = true;
        q += 65;
      }
    } else if (m == 0xDD) {
      if (sl != 2) return kCorrupt;
      hd->ri = (seg[0] << 8) | seg[1];
    } else if (m == 0xEE) {
      if (sl >= 12 && memcmp(seg, "Adobe", 5) == 0) return kUnsupported;
    } else if (m == 0xDA) {
      if (!have_sof || sl < 1) return kCorrupt;
      const int ns = seg[0];
      if (sl != 4 + 2 * (size_t)ns || ns < 1 || ns > 4) return kCorrupt;
      if (ns != hd->ncomp) return kUnsupported;  // several scans
      for (int i = 0; i < ns; ++i)
        if (seg[1 + 2 * i] != hd->ids[i]) return kUnsupported;
      for (int i = 0; i < ns; ++i) {
        hd->td[i] = seg[2 + 2 * i] >> 4;
        hd->ta[i] = seg[2 + 2 * i] & 15;
      }
      if (seg[1 + 2 * ns] != 0 || seg[2 + 2 * ns] != 63 || seg[3 + 2 * ns] != 0) return kCorrupt;
      for (int i = 0; i < ns; ++i)
        if (hd->td[i] > 3 || hd->ta[i] > 3 || !hd->huff[0][hd->td[i]].present || !hd->huff[1][hd->ta[i]].present ||
            !hd->have_qt[hd->tq[i]])
          return kCorrupt;  // a missing table
      const int mx = (hd->w + 8 * hd->hs - 1) / (8 * hd->hs), my = (hd->h + 8 * hd->vs - 1) / (8 * hd->vs);
      hd->blocks = 0;
      for (int i = 0; i < hd->ncomp; ++i) {
        hd->bw[i] = i ? mx : mx * hd->hs;
        hd->bh[i] = i ? my : my * hd->vs;
        hd->blocks += (int64_t)hd->bw[i] * hd->bh[i];
      }
      if (hd->blocks > 4 * (int64_t)(n - p)) return kCorrupt;  // a block takes two bits at the least
      hd->scan = p;
      return kOk;
    }
    // APPn, COM: skipped
  }
}

// The entropy-coded segment as a bit stream: byte stuffing removed, fill bytes skipped; at a marker
// or the end of the data the buffer is padded with zeros, and consuming a padding bit fails.
struct Bits {
  const uint8_t* d;
  size_t n, p;
  uint64_t acc = 0;
  int cnt = 0, pad = 0;
  bool end = false;
  Bits(const uint8_t* data, size_t bytes, size_t at) : d(data), n(bytes), p(at) {}
  void fill() {
    while (cnt <= 56) {
      uint64_t b = 0;
      while (!end) {
        if (p >= n) {
          end = true;
        } else if (d[p] != 0xFF) {
          b = d[p++];
          break;
        } else if (p + 1 >= n) {
          end = true;
        } else if (d[p + 1] == 0x00) {
          b = 0xFF;
          p += 2;
          break;
        } else if (d[p + 1] == 0xFF) {
          ++p;  // a fill byte
        } else {
          end = true;  // a marker: p stays on its 0xFF
        }
      }
      if (end) pad += 8;
      acc = (acc << 8) | b;
      cnt += 8;
    }
  }
  uint32_t peek(int k) const { return (uint32_t)(acc >> (cnt - k)) & ((1u << k) - 1u); }
  bool take(int k) {
    cnt -= k;
    return cnt >= pad;
  }
  // -1: an undefined code or the end of the data
  int decode(const Huff& t) {
    if (cnt < 32) fill();
    const uint32_t look = peek(kLook);
    int len = t.look_len[look];
    if (len) return take(len) ? t.look_sym[look] : -1;
    len = kLook + 1;
    int32_t code = (int32_t)peek(len);
    while (code > t.maxcode[len]) code = (int32_t)peek(++len);
    if (len > 16 || !take(len)) return -1;
    return t.sym[(code + t.valoff[len]) & 255];
  }
  // s bits (1 .. 15), EXTENDed; false at the end of the data
  bool receive_extend(int s, int32_t* v) {
    if (cnt < 32) fill();
    const int32_t r = (int32_t)peek(s);
    *v = r < (1 << (s - 1)) ? r - (1 << s) + 1 : r;
    return take(s);
  }
  // the marker at the next byte boundary, consumed: -1 without one
  int marker() {
    fill();
    if (!end || cnt - pad >= 8 || p + 1 >= n) return -1;
    const int m = d[p + 1];
    p += 2;
    acc = 0;
    cnt = pad = 0;
    end = false;
    return m;
  }
};

// The predicate of one block in natural order (jpeg.py in_range)
inline bool block_in_range(const int16_t* coef, const uint16_t* q) {
  int64_t mag = 0;
  for (int k = 0; k < 64; ++k) {
    const int64_t v = (int64_t)coef[k] * q[k];
    mag += v < 0 ? -v : v;
  }
  return mag <= kRangeSum;
}

// The scan of a parsed file into coef: hd.blocks blocks of 64 int16 in natural order, component
// after component, each in raster order over its padded grid.  -> kOk, kRange or kCorrupt
inline int decode_scan(const uint8_t* d, size_t n, const Header& hd, int16_t* coef) {
  Bits br(d, n, hd.scan);
  int16_t* base[3];
  int64_t off = 0;
  for (int c = 0; c < hd.ncomp; ++c) {
    base[c] = coef + off * 64;
    off += (int64_t)hd.bw[c] * hd.bh[c];
  }
  const int mx = hd.ncomp > 1 ? hd.bw[1] : hd.bw[0], my = hd.ncomp > 1 ? hd.bh[1] : hd.bh[0];
  int32_t pred[3] = {0, 0, 0};
  bool in_range = true;
  int64_t mcu = 0;
  int rst = 0;
  for (int row = 0; row < my; ++row) {
    for (int col = 0; col < mx; ++col, ++mcu) {
      if (hd.ri && mcu && mcu % hd.ri == 0) {
        if (br.marker() != 0xD0 + (rst & 7)) return kCorrupt;
        ++rst;
        pred[0] = pred[1] = pred[2] = 0;
      }
      for (int c = 0; c < hd.ncomp; ++c) {
        const Huff& dc = hd.huff[0][hd.td[c]];
        const Huff& ac = hd.huff[1][hd.ta[c]];
        const uint16_t* q = hd.qt[hd.tq[c]];
        const int ch = c ? 1 : hd.hs, cv = c ? 1 : hd.vs;
        for (int v = 0; v < cv; ++v) {
          for (int u = 0; u < ch; ++u) {
            int16_t* blk = base[c] + ((int64_t)(row * cv + v) * hd.bw[c] + col * ch + u) * 64;
            memset(blk, 0, 128);
            int s = br.decode(dc);
            if (s < 0) return kCorrupt;
            if (s) {
              int32_t diff;
              if (!br.receive_extend(s, &diff)) return kCorrupt;
              pred[c] += diff;
            }
            if (pred[c] < -32768 || pred[c] > 32767) return kCorrupt;
            blk[0] = (int16_t)pred[c];
            int64_t mag = (int64_t)(pred[c] < 0 ? -pred[c] : pred[c]) * q[0];
            int k = 1;
            while (k < 64) {
              const int rs = br.decode(ac);
              if (rs < 0) return kCorrupt;
              const int r = rs >> 4;
              s = rs & 15;
              if (s == 0) {
                if (r != 15) break;
                k += 16;
                if (k > 64) return kCorrupt;
                continue;
              }
              k += r;
              if (k > 63) return kCorrupt;
              int32_t val;
              if (!br.receive_extend(s, &val)) return kCorrupt;
              const int at = kZigzag[k];
              blk[at] = (int16_t)val;
              mag += (int64_t)(val < 0 ? -val : val) * q[at];
              ++k;
            }
            if (mag > kRangeSum) in_range = false;
          }
        }
      }
    }
  }
  if (br.marker() != 0xD9) return kCorrupt;
  return in_range ? kOk : kRange;
}

// ---- the batch ----
inline std::atomic<int>& pool_threads() {
  static std::atomic<int> t{0};  // 0: the default
  return t;
}

// min(16, hardware_concurrency()) unless set (1 .. 64): never the machine's whole core count
inline int batch_threads() {
  const int set = pool_threads().load();
  if (set > 0) return set;
  const unsigned hc = std::thread::hardware_concurrency();
  return hc == 0 ? 1 : (hc < 16 ? (int)hc : 16);
}

struct Task {
  const uint8_t* data;
  size_t bytes;
  int16_t* coef;  // sized from the header this file parsed to before
  int status;     // in: kOk to decode; out: the decode's
};

// Header parse and scan of one file whose header parsed before (the tables are rebuilt here, on the
// worker's stack, and do not wait in memory per frame of the batch)
inline int decode_file(const uint8_t* d, size_t n, int16_t* coef) {
  Header hd;
  const int st = parse_header(d, n, &hd);
  return st != kOk ? st : decode_scan(d, n, hd, coef);
}

// Decodes every task whose status is kOk, a frame at a time per thread, min(tasks, threads) workers
inline void decode_batch(Task* tasks, int n) {
  int todo = 0;
  for (int i = 0; i < n; ++i) todo += tasks[i].status == kOk;
  if (!todo) return;
  std::atomic<int> next{0};
  auto work = [&] {
    for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1))
      if (tasks[i].status == kOk) tasks[i].status = decode_file(tasks[i].data, tasks[i].bytes, tasks[i].coef);
  };
  const int threads = batch_threads() < todo ? batch_threads() : todo;
  std::vector<std::thread> pool;
  try {
    pool.reserve((size_t)threads);
    for (int t = 1; t < threads; ++t) pool.emplace_back(work);
  } catch (...) {  // no thread to be had: the ones that started, and this one, do the work
  }
  work();
  for (std::thread& t : pool) t.join();
}

}  // namespace jpeg
}  // namespace op
