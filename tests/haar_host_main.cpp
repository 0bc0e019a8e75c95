// csrc/haar_host.hpp on its own (no GPU, no library): groups seeded rectangles and lists the scales
// of a few frames; tests/test_haar_host_main.py builds this plainly and under ASan/UBSan and compares
// every line with haar.py's statement.
//   haar_host_main SEED COUNT
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "haar_host.hpp"

using namespace op::haar;

static uint32_t g_state;
static uint32_t next() {  // a 31-bit LCG: the test needs only the printed rectangles
  g_state = g_state * 1103515245u + 12345u;
  return (g_state >> 8) & 0xffffu;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  g_state = (uint32_t)std::atoi(argv[1]);
  const int count = std::atoi(argv[2]);
  // clusters of jittered squares of a few sizes, small ones inside large ones, and strays
  std::vector<Rect> rects;
  for (int i = 0; i < count; ++i) {
    const int cluster = (int)(next() % 7u), size = 20 + 12 * (cluster % 4);
    const int cx = 40 + 90 * (cluster % 3), cy = 40 + 70 * (cluster / 3);
    const int jitter = 1 + size / 6;
    Rect r{cx + (int)(next() % (unsigned)jitter), cy + (int)(next() % (unsigned)jitter), size + (int)(next() % 4u),
           size + (int)(next() % 4u)};
    if (next() % 11u == 0) r = Rect{(int)(next() % 400u), (int)(next() % 300u), 10 + (int)(next() % 50u), 10 + (int)(next() % 50u)};
    rects.push_back(r);
    std::printf("in %d %d %d %d\n", r.x, r.y, r.w, r.h);
  }
  std::vector<Rect> out;
  std::vector<int32_t> neighbours;
  for (int min_neighbors : {0, 1, 3, 6}) {
    group_rectangles(rects, min_neighbors, 0.2, &out, &neighbours);
    if (out.size() != neighbours.size()) return 3;
    for (size_t i = 0; i < out.size(); ++i)
      std::printf("group %d %d %d %d %d %d\n", min_neighbors, out[i].x, out[i].y, out[i].w, out[i].h, neighbours[i]);
  }
  group_rectangles(std::vector<Rect>(), 3, 0.2, &out, &neighbours);
  if (!out.empty() || !neighbours.empty()) return 4;
  const int frames[][2] = {{48, 64}, {20, 20}, {30, 19}, {480, 640}, {584, 584}, {16384, 16384}};
  const double factors[] = {1.2, 1.1, 1.01};
  std::vector<Scale> sc;
  for (const auto& f : frames)
    for (double factor : factors) {
      const bool ok = scales(f[0], f[1], 20, 20, factor, 1, 1, f[1], f[0], &sc);
      std::printf("scales %d %d %.17g %d", f[0], f[1], factor, ok ? (int)sc.size() : -1);
      if (ok)
        for (const Scale& s : sc) std::printf(" %.9g:%d:%d", (double)s.sc, s.lw, s.lh);
      std::printf("\n");
    }
  std::printf("haar host ok\n");
  return 0;
}
