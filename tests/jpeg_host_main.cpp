// Drives csrc/jpeg_host.hpp over hostile input with no GPU and no library: for every file named on
// the command line, every prefix of it, and the file with every stride-th byte replaced by 0x00,
// 0xFF and its complement, goes through the header parse and the entropy decode.  Every call must
// return a status; tests/test_jpeg_host_asan.py builds this with -fsanitize=address,undefined, so a
// read or write out of bounds, an overflow or a leak ends the run.
//   jpeg_host_main <stride> <file>...
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "jpeg_host.hpp"

static long g_calls = 0, g_ok = 0;

static int run(const std::vector<uint8_t>& d, size_t n) {
  // the bytes are copied into an allocation of exactly n, so a read past the end is seen
  std::vector<uint8_t> exact(d.begin(), d.begin() + (long)n);
  op::jpeg::Header hd;
  int st = op::jpeg::parse_header(exact.data(), n, &hd);
  ++g_calls;
  if (st == op::jpeg::kOk) {
    if (hd.h < 1 || hd.h > op::jpeg::kMaxSide || hd.w < 1 || hd.w > op::jpeg::kMaxSide || hd.blocks > 4 * (long)n) {
      fprintf(stderr, "a header outside the validated bounds\n");
      exit(2);
    }
    std::vector<int16_t> coef((size_t)hd.blocks * 64);
    st = op::jpeg::decode_scan(exact.data(), n, hd, coef.data());
  }
  if (st < 0 || st > op::jpeg::kRange) {
    fprintf(stderr, "status %d\n", st);
    exit(2);
  }
  g_ok += st == op::jpeg::kOk;
  return st;
}

int main(int argc, char** argv) {
  if (argc < 3) return 1;
  const size_t stride = (size_t)atoi(argv[1]);
  if (stride < 1) return 1;
  for (int a = 2; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) return 1;
    std::vector<uint8_t> d;
    uint8_t buf[4096];
    for (size_t got; (got = fread(buf, 1, sizeof(buf), f)) > 0;) d.insert(d.end(), buf, buf + got);
    fclose(f);
    if (run(d, d.size()) != op::jpeg::kOk) {
      fprintf(stderr, "%s does not decode\n", argv[a]);
      return 2;
    }
    for (size_t n = 0; n < d.size(); ++n)
      if (run(d, n) == op::jpeg::kOk) {
        fprintf(stderr, "%s: a prefix of %zu bytes decodes\n", argv[a], n);
        return 2;
      }
    for (size_t i = 0; i < d.size(); i += stride) {
      const uint8_t keep = d[i];
      const uint8_t with[3] = {0x00, 0xFF, (uint8_t)~keep};
      for (uint8_t v : with) {
        d[i] = v;
        run(d, d.size());
      }
      d[i] = keep;
    }
  }
  // the batch pool: the first file eight times over, every other one cut short, four threads
  {
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 1;
    std::vector<uint8_t> d(1 << 16);
    d.resize(fread(d.data(), 1, d.size(), f));
    fclose(f);
    op::jpeg::Header hd;
    if (op::jpeg::parse_header(d.data(), d.size(), &hd) != op::jpeg::kOk) return 2;
    std::vector<int16_t> coef((size_t)hd.blocks * 64 * 8);
    std::vector<op::jpeg::Task> tasks;
    for (int i = 0; i < 8; ++i)
      tasks.push_back(op::jpeg::Task{d.data(), i % 2 ? d.size() - 9 : d.size(), coef.data() + (size_t)hd.blocks * 64 * i, op::jpeg::kOk});
    op::jpeg::pool_threads().store(4);
    op::jpeg::decode_batch(tasks.data(), 8);
    for (int i = 0; i < 8; ++i)
      if (tasks[i].status != (i % 2 ? op::jpeg::kCorrupt : op::jpeg::kOk)) {
        fprintf(stderr, "batch: task %d has status %d\n", i, tasks[i].status);
        return 2;
      }
    for (int i = 2; i < 8; i += 2)
      if (memcmp(coef.data(), coef.data() + (size_t)hd.blocks * 64 * i, (size_t)hd.blocks * 128) != 0) return 2;
  }
  printf("jpeg host ok: %ld calls, %ld decoded\n", g_calls, g_ok);
  return 0;
}
