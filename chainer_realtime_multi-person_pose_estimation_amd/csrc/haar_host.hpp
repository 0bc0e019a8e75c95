// The host half of the Haar cascade detector (haar.py states it in NumPy): the scale list of a frame
// and cv::groupRectangles.  Plain C++17, no HIP: haar.hip includes it, and so does the stand-alone
// program tests/haar_host_main.cpp (built plain and under ASan/UBSan).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <vector>

namespace op {
namespace haar {

constexpr int kMaxWindow = 64;   // largest window side
constexpr int kMaxScales = 64;   // most layers of one frame
constexpr int kMaxSide = 16384;  // largest frame side

struct Rect {
  int32_t x, y, w, h;
};

struct Scale {
  float sc;        // float32(factor)
  int32_t lw, lh;  // rint(w / sc), rint(h / sc)
};

// rint, half to even (the default rounding mode; nothing here changes it)
inline int32_t rint_i(double v) { return (int32_t)std::nearbyint(v); }

// haar.scales: false when the frame has more than kMaxScales scales.  scale_factor >= 1.01 (checked by
// the caller) bounds the loop: the window passes 16384 after at most 980 steps.
inline bool scales(int h, int w, int win_w, int win_h, double scale_factor, int min_w, int min_h, int max_w, int max_h,
                   std::vector<Scale>* out) {
  out->clear();
  for (double factor = 1.0;; factor *= scale_factor) {
    const int32_t ww = rint_i(win_w * factor), wh = rint_i(win_h * factor);
    if (ww > max_w || wh > max_h || ww > w || wh > h) return true;
    if (ww < min_w || wh < min_h) continue;
    if ((int)out->size() == kMaxScales) return false;
    const float sc = (float)factor;
    out->push_back(Scale{sc, rint_i((double)w / (double)sc), rint_i((double)h / (double)sc)});
  }
}

inline bool similar(const Rect& a, const Rect& b, double eps) {
  const double delta = eps * (std::min(a.w, b.w) + std::min(a.h, b.h)) * 0.5;
  return std::abs(a.x - b.x) <= delta && std::abs(a.y - b.y) <= delta && std::abs(a.x + a.w - b.x - b.w) <= delta &&
         std::abs(a.y + a.h - b.y - b.h) <= delta;
}

// cv::groupRectangles (haar.group_rectangles_np): connected components under `similar`, numbered by
// their first member; a class's rectangle is its integer sums times float32(1 / count), rounded half to
// even; classes of at most min_neighbors members go, and so does a rectangle inside a stronger one.
// min_neighbors <= 0: the input, one neighbour each.
inline void group_rectangles(const std::vector<Rect>& in, int min_neighbors, double eps, std::vector<Rect>* out,
                             std::vector<int32_t>* neighbours) {
  out->clear();
  neighbours->clear();
  const int n = (int)in.size();
  if (min_neighbors <= 0 || n == 0) {
    *out = in;
    neighbours->assign((size_t)n, 1);
    return;
  }
  std::vector<int> parent((size_t)n);
  for (int i = 0; i < n; ++i) parent[i] = i;
  auto root = [&](int i) {
    while (parent[i] != i) {
      parent[i] = parent[parent[i]];
      i = parent[i];
    }
    return i;
  };
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j)
      if (similar(in[i], in[j], eps)) {
        const int a = root(i), b = root(j);
        if (a != b) parent[std::max(a, b)] = std::min(a, b);
      }
  std::vector<int> label((size_t)n, -1);
  std::vector<int64_t> sum;  // 4 per class
  std::vector<int32_t> count;
  for (int i = 0; i < n; ++i) {
    const int r = root(i);  // the smallest member: first met at i == r
    if (label[r] < 0) {
      label[r] = (int)count.size();
      count.push_back(0);
      sum.insert(sum.end(), 4, 0);
    }
    const int c = label[r];
    count[c] += 1;
    sum[4 * c] += in[i].x;
    sum[4 * c + 1] += in[i].y;
    sum[4 * c + 2] += in[i].w;
    sum[4 * c + 3] += in[i].h;
  }
  const int nc = (int)count.size();
  std::vector<Rect> mean((size_t)nc);
  for (int c = 0; c < nc; ++c) {
    const float inv = 1.0f / (float)count[c];
    auto avg = [&](int64_t s) { return (int32_t)std::nearbyint((float)s * inv); };
    mean[c] = Rect{avg(sum[4 * c]), avg(sum[4 * c + 1]), avg(sum[4 * c + 2]), avg(sum[4 * c + 3])};
  }
  for (int i = 0; i < nc; ++i) {
    const Rect& r1 = mean[i];
    const int n1 = count[i];
    if (n1 <= min_neighbors) continue;
    int j = 0;
    for (; j < nc; ++j) {
      const int n2 = count[j];
      if (j == i || n2 <= min_neighbors) continue;
      const Rect& r2 = mean[j];
      const int dx = (int)(r2.w * eps), dy = (int)(r2.h * eps);
      if (r1.x >= r2.x - dx && r1.y >= r2.y - dy && r1.x + r1.w <= r2.x + r2.w + dx && r1.y + r1.h <= r2.y + r2.h + dy &&
          (n2 > std::max(3, n1) || n1 < 3))
        break;
    }
    if (j == nc) {
      out->push_back(r1);
      neighbours->push_back(n1);
    }
  }
}

}  // namespace haar
}  // namespace op
