// Host check of the IVF probe under a user filter: the size functions and every argument error of
// dewi_ivf_probe_prepare_filtered, which abi.cpp raises before any device work.  A program of its own, so that abi.cpp can be
// compiled with the host sanitizers and run without a GPU:  make hostcheck  (csrc/Makefile) builds and runs it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../include/dewi_hip.h"

static int failures = 0;

#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);          \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

int main() {
  EXPECT(dewi_abi_version() == DEWI_ABI_VERSION);

  // sizes: positive multiples of 4 bytes, never below the unfiltered probe's, 0 for a bad shape
  const int64_t rows[] = {1, 100, 600, 20000, int64_t{1} << 20, 0xFFFFFFFFll};
  const int dims[] = {5, 50, 64, 129, 768};
  const int groups[] = {1, 8, 32};
  for (int64_t n : rows)
    for (int dim : dims)
      for (int group : groups) {
        const size_t stride = dewi_ivf_probe_filtered_group_bytes(n, dim, 0, group);
        EXPECT(stride > 0 && stride % 4 == 0);
        EXPECT(stride >= dewi_ivf_probe_group_bytes(n, dim, 0, group));
        const int batches[] = {1, group, group + 1, 4 * group, 65535};
        for (int b : batches) {
          const size_t need = dewi_ivf_probe_filtered_bytes(n, dim, 0, b, group);
          const size_t n_groups = static_cast<size_t>((b + group - 1) / group);
          EXPECT(need > 0 && need % 4 == 0);
          EXPECT(need >= dewi_ivf_probe_bytes(n, dim, 0, b, group));
          EXPECT(need >= n_groups * stride + 4 * (n_groups + static_cast<size_t>(b)));
        }
      }
  EXPECT(dewi_ivf_probe_filtered_bytes(0, 64, 0, 4, 8) == 0);
  EXPECT(dewi_ivf_probe_filtered_bytes(-5, 64, 0, 4, 8) == 0);
  EXPECT(dewi_ivf_probe_filtered_bytes(int64_t{1} << 33, 64, 0, 4, 8) == 0);
  EXPECT(dewi_ivf_probe_filtered_bytes(100, 0, 0, 4, 8) == 0);
  EXPECT(dewi_ivf_probe_filtered_bytes(100, 64, 2, 4, 8) == 0);
  EXPECT(dewi_ivf_probe_filtered_bytes(100, 64, 0, 0, 8) == 0);
  EXPECT(dewi_ivf_probe_filtered_bytes(100, 64, 0, 65536, 8) == 0);
  EXPECT(dewi_ivf_probe_filtered_bytes(100, 64, 0, 4, 0) == 0);
  EXPECT(dewi_ivf_probe_filtered_bytes(100, 64, 0, 4, 33) == 0);
  EXPECT(dewi_ivf_probe_filtered_group_bytes(100, 64, 0, 33) == 0);
  EXPECT(dewi_ivf_probe_filtered_group_bytes(0, 64, 0, 8) == 0);

  // argument errors: none of these calls reaches the device (the pointers are host memory nobody reads)
  alignas(16) static unsigned char dummy[64];
  void* p = dummy;
  const int64_t* ids = reinterpret_cast<const int64_t*>(dummy);
  const uint8_t* allow = dummy;
  int64_t cnt[4] = {0, 0, 0, 0};
  const size_t big = size_t{1} << 20;
  EXPECT(dewi_ivf_probe_prepare_filtered(1, 100, 64, p, 4, ids, 2, 1, 8, allow, 0, p, big, cnt, cnt, nullptr) == DEWI_ERR_UNSUPPORTED);
  EXPECT(dewi_ivf_probe_prepare_filtered(0, 100, 64, nullptr, 4, ids, 2, 1, 8, allow, 0, p, big, cnt, cnt, nullptr) == DEWI_ERR_INVALID_ARG);
  EXPECT(dewi_ivf_probe_prepare_filtered(0, 100, 64, p, 4, nullptr, 2, 1, 8, allow, 0, p, big, cnt, cnt, nullptr) == DEWI_ERR_INVALID_ARG);
  EXPECT(dewi_ivf_probe_prepare_filtered(0, 100, 64, p, 4, ids, 2, 1, 8, nullptr, 0, p, big, cnt, cnt, nullptr) == DEWI_ERR_INVALID_ARG);
  EXPECT(dewi_ivf_probe_prepare_filtered(0, 100, 64, p, 4, ids, 2, 1, 8, allow, 0, nullptr, big, cnt, cnt, nullptr) == DEWI_ERR_INVALID_ARG);
  EXPECT(dewi_ivf_probe_prepare_filtered(0, 100, 64, p, 4, ids, 2, 1, 8, allow, 0, p, big, nullptr, cnt, nullptr) == DEWI_ERR_INVALID_ARG);
  EXPECT(dewi_ivf_probe_prepare_filtered(0, 100, 64, p, 4, ids, 2, 1, 8, allow, 0, p, big, cnt, nullptr, nullptr) == DEWI_ERR_INVALID_ARG);
  EXPECT(dewi_ivf_probe_prepare_filtered(0, 0, 64, p, 4, ids, 2, 1, 8, allow, 0, p, big, cnt, cnt, nullptr) != DEWI_OK);
  EXPECT(dewi_ivf_probe_prepare_filtered(0, 100, 0, p, 4, ids, 2, 1, 8, allow, 0, p, big, cnt, cnt, nullptr) != DEWI_OK);
  EXPECT(dewi_ivf_probe_prepare_filtered(0, 100, 64, p, 0, ids, 2, 1, 8, allow, 0, p, big, cnt, cnt, nullptr) == DEWI_ERR_INVALID_ARG);
  EXPECT(dewi_ivf_probe_prepare_filtered(0, 100, 64, p, 101, ids, 2, 1, 8, allow, 0, p, big, cnt, cnt, nullptr) == DEWI_ERR_INVALID_ARG);
  EXPECT(dewi_ivf_probe_prepare_filtered(0, 100, 64, p, 4, ids, 0, 1, 8, allow, 0, p, big, cnt, cnt, nullptr) == DEWI_ERR_INVALID_ARG);
  EXPECT(dewi_ivf_probe_prepare_filtered(0, 100, 64, p, 4, ids, 65536, 1, 8, allow, 0, p, big, cnt, cnt, nullptr) == DEWI_ERR_INVALID_ARG);
  EXPECT(dewi_ivf_probe_prepare_filtered(0, 100, 64, p, 4, ids, 2, 0, 8, allow, 0, p, big, cnt, cnt, nullptr) == DEWI_ERR_INVALID_ARG);
  EXPECT(dewi_ivf_probe_prepare_filtered(0, 100, 64, p, 4, ids, 2, 5, 8, allow, 0, p, big, cnt, cnt, nullptr) == DEWI_ERR_INVALID_ARG);
  EXPECT(dewi_ivf_probe_prepare_filtered(0, 100, 64, p, 4, ids, 2, 1, 0, allow, 0, p, big, cnt, cnt, nullptr) == DEWI_ERR_INVALID_ARG);
  EXPECT(dewi_ivf_probe_prepare_filtered(0, 100, 64, p, 4, ids, 2, 1, 33, allow, 0, p, big, cnt, cnt, nullptr) == DEWI_ERR_INVALID_ARG);
  EXPECT(dewi_ivf_probe_prepare_filtered(0, 100, 64, p, 4, ids, 2, 1, 8, allow, 2, p, big, cnt, cnt, nullptr) == DEWI_ERR_INVALID_ARG);
  EXPECT(dewi_ivf_probe_prepare_filtered(0, 100, 64, p, 4, ids, 2, 1, 8, allow, -1, p, big, cnt, cnt, nullptr) == DEWI_ERR_INVALID_ARG);
  const size_t need = dewi_ivf_probe_filtered_bytes(100, 64, 0, 2, 8);
  EXPECT(dewi_ivf_probe_prepare_filtered(0, 100, 64, p, 4, ids, 2, 1, 8, allow, 0, p, need - 1, cnt, cnt, nullptr) == DEWI_ERR_WORKSPACE);
  EXPECT(dewi_ivf_probe_prepare_filtered(0, 100, 64, p, 4, ids, 2, 1, 8, allow, 1, p, 0, cnt, cnt, nullptr) == DEWI_ERR_WORKSPACE);
  EXPECT(dewi_ivf_probe_prepare_filtered(0, 100, 64, p, 4, ids, 2, 1, 8, allow, 0, p, dewi_ivf_probe_bytes(100, 64, 0, 2, 8), cnt, cnt,
                                         nullptr) == DEWI_ERR_WORKSPACE);
  EXPECT(cnt[0] == 0 && cnt[1] == 0 && cnt[2] == 0 && cnt[3] == 0);   // a refused call writes no count

  if (failures) {
    std::fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  std::puts("hostcheck_ivf_filtered: ok");
  return 0;
}
