// Host check of the search by examples: the argument checks of dewi_knn_candidates_examples, which abi.cpp makes before any
// device work, and the arithmetic of dewi_knn_examples_workspace_bytes, which needs no device.  A program of its own that needs
// no GPU:  make hostcheck  (csrc/Makefile) builds and runs it under the host sanitizers.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <limits>

#include "../../include/dewi_hip.h"

static int failures = 0;

#define EXPECT(cond)                                          \
  do {                                                        \
    if (!(cond)) {                                            \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
      ++failures;                                             \
    }                                                         \
  } while (0)

alignas(16) static unsigned char dummy[64];   // stands for device memory: nobody reads it, no call here reaches the device

struct Args {
  const float* E = reinterpret_cast<const float*>(dummy);
  int64_t n_rows = 1000;
  int dim = 768;
  const float* X = reinterpret_cast<const float*>(dummy);
  int n_pos = 2, n_neg = 1, match = DEWI_EXAMPLES_MATCH_ANY, rule = DEWI_EXAMPLES_RULE_PENALTY;
  double weight = 1.0;
  const int64_t* exclude = nullptr;
  int n_exclude = 0;
  const void* filter = nullptr;
  int64_t n_allowed = 0;
  const float* dewi = reinterpret_cast<const float*>(dummy);
  const float* ent = reinterpret_cast<const float*>(dummy);
  int c = 20;
  int64_t id_offset = 0;
  dewi_candidate* out = reinterpret_cast<dewi_candidate*>(dummy);
  void* ws = nullptr;          // every call below must fail (or return) before the workspace is looked at, or on it
  size_t ws_bytes = 0;
};

static int run(const Args& a) {
  return dewi_knn_candidates_examples(a.E, a.n_rows, a.dim, a.X, a.n_pos, a.n_neg, a.match, a.rule, a.weight, a.exclude, a.n_exclude,
                                      a.filter, a.n_allowed, a.dewi, a.ent, a.c, a.id_offset, a.out, a.ws, a.ws_bytes, nullptr);
}

int main() {
  const double inf = std::numeric_limits<double>::infinity();
  // ---- argument errors, each before any device work; with everything else valid the call stops at the (missing) workspace
  EXPECT(run(Args{}) == DEWI_ERR_WORKSPACE);
  { Args a; a.E = nullptr; EXPECT(run(a) == DEWI_ERR_INVALID_ARG); }
  { Args a; a.X = nullptr; EXPECT(run(a) == DEWI_ERR_INVALID_ARG); }
  { Args a; a.dewi = nullptr; EXPECT(run(a) == DEWI_ERR_INVALID_ARG); }
  { Args a; a.ent = nullptr; EXPECT(run(a) == DEWI_ERR_INVALID_ARG); }
  { Args a; a.out = nullptr; EXPECT(run(a) == DEWI_ERR_INVALID_ARG); }
  { Args a; a.n_rows = 0; EXPECT(run(a) == DEWI_ERR_INVALID_ARG); }
  { Args a; a.n_rows = -1; EXPECT(run(a) == DEWI_ERR_INVALID_ARG); }
  { Args a; a.n_rows = int64_t{1} << 32; EXPECT(run(a) == DEWI_ERR_UNSUPPORTED); }
  { Args a; a.dim = 0; EXPECT(run(a) == DEWI_ERR_INVALID_ARG); }
  { Args a; a.n_pos = 0; EXPECT(run(a) == DEWI_ERR_INVALID_ARG); }
  { Args a; a.n_pos = -2; EXPECT(run(a) == DEWI_ERR_INVALID_ARG); }
  { Args a; a.n_neg = -1; EXPECT(run(a) == DEWI_ERR_INVALID_ARG); }
  { Args a; a.n_pos = 16; a.n_neg = 0; EXPECT(run(a) == DEWI_ERR_WORKSPACE); }                 // exactly full: valid
  { Args a; a.n_pos = 8; a.n_neg = 9; EXPECT(run(a) == DEWI_ERR_UNSUPPORTED); }
  { Args a; a.n_pos = std::numeric_limits<int>::max(); a.n_neg = std::numeric_limits<int>::max(); EXPECT(run(a) == DEWI_ERR_UNSUPPORTED); }
  { Args a; a.match = 2; EXPECT(run(a) == DEWI_ERR_INVALID_ARG); }
  { Args a; a.match = -1; EXPECT(run(a) == DEWI_ERR_INVALID_ARG); }
  { Args a; a.rule = 2; EXPECT(run(a) == DEWI_ERR_INVALID_ARG); }
  { Args a; a.weight = std::nan(""); EXPECT(run(a) == DEWI_ERR_INVALID_ARG); }
  { Args a; a.weight = inf; EXPECT(run(a) == DEWI_ERR_INVALID_ARG); }
  { Args a; a.weight = -inf; EXPECT(run(a) == DEWI_ERR_INVALID_ARG); }
  { Args a; a.weight = 1e39; EXPECT(run(a) == DEWI_ERR_INVALID_ARG); }                        // not finite in fp32
  { Args a; a.weight = -3.5; EXPECT(run(a) == DEWI_ERR_WORKSPACE); }                          // any finite weight is valid
  { Args a; a.n_exclude = -1; EXPECT(run(a) == DEWI_ERR_INVALID_ARG); }
  { Args a; a.n_exclude = DEWI_EXAMPLES_MAX + 1; a.exclude = reinterpret_cast<const int64_t*>(dummy); EXPECT(run(a) == DEWI_ERR_INVALID_ARG); }
  { Args a; a.n_exclude = 1; EXPECT(run(a) == DEWI_ERR_INVALID_ARG); }                        // NULL d_exclude
  { Args a; a.n_exclude = DEWI_EXAMPLES_MAX; a.exclude = reinterpret_cast<const int64_t*>(dummy); EXPECT(run(a) == DEWI_ERR_WORKSPACE); }
  { Args a; a.filter = dummy; a.n_allowed = -1; EXPECT(run(a) == DEWI_ERR_INVALID_ARG); }
  { Args a; a.filter = dummy; a.n_allowed = 1001; EXPECT(run(a) == DEWI_ERR_INVALID_ARG); }
  { Args a; a.filter = dummy; a.n_allowed = 0; EXPECT(run(a) == DEWI_OK); }                   // nothing launched, nothing written
  { Args a; a.filter = dummy; a.n_allowed = 1000; EXPECT(run(a) == DEWI_ERR_WORKSPACE); }
  { Args a; a.c = 0; EXPECT(run(a) == DEWI_ERR_INVALID_ARG); }
  { Args a; a.c = -7; EXPECT(run(a) == DEWI_ERR_INVALID_ARG); }
  { Args a; a.c = 2049; EXPECT(run(a) == DEWI_ERR_UNSUPPORTED); }
  { Args a; a.c = 2048; EXPECT(run(a) == DEWI_ERR_WORKSPACE); }
  for (int dim : {4, 64, 128, 130, 133, 766, 4097, 4100, 1 << 20}) {
    Args a;
    a.dim = dim;
    EXPECT(run(a) == DEWI_ERR_UNSUPPORTED);
  }
  for (int dim : {132, 256, 388, 768, 1000, 1536, 2052, 4096}) {
    Args a;
    a.dim = dim;
    EXPECT(run(a) == DEWI_ERR_WORKSPACE);
  }
  { Args a; a.id_offset = -1; EXPECT(run(a) == DEWI_ERR_UNSUPPORTED); }
  { Args a; a.id_offset = 0x7FFFFFFFll - 999; EXPECT(run(a) == DEWI_ERR_UNSUPPORTED); }
  { Args a; a.id_offset = 0x7FFFFFFFll - 1000; EXPECT(run(a) == DEWI_ERR_WORKSPACE); }
  { Args a; a.id_offset = std::numeric_limits<int64_t>::max() - 1000; EXPECT(run(a) == DEWI_ERR_UNSUPPORTED); }
  { Args a; a.ws = dummy; a.ws_bytes = dewi_knn_examples_workspace_bytes(1000, 768, 3, 20) - 1; EXPECT(run(a) == DEWI_ERR_WORKSPACE); }
  EXPECT(dewi_examples_tuning_set(-1) == DEWI_ERR_INVALID_ARG);
  EXPECT(dewi_examples_tuning_set(3) == DEWI_OK);
  EXPECT(dewi_examples_tuning_set(0) == DEWI_OK);

  // ---- the workspace arithmetic: 0 for what the route does not take, otherwise the keys and 8 bytes per scanned row
  EXPECT(dewi_knn_examples_workspace_bytes(0, 768, 1, 10) == 0);
  EXPECT(dewi_knn_examples_workspace_bytes(-1, 768, 1, 10) == 0);
  EXPECT(dewi_knn_examples_workspace_bytes((int64_t{1} << 32), 768, 1, 10) == 0);
  EXPECT(dewi_knn_examples_workspace_bytes(1000, 768, 0, 10) == 0);
  EXPECT(dewi_knn_examples_workspace_bytes(1000, 768, DEWI_EXAMPLES_MAX + 1, 10) == 0);
  EXPECT(dewi_knn_examples_workspace_bytes(1000, 768, 1, 0) == 0);
  EXPECT(dewi_knn_examples_workspace_bytes(1000, 768, 1, 2049) == 0);
  for (int dim : {-4, 0, 3, 128, 130, 4100, std::numeric_limits<int>::max()}) EXPECT(dewi_knn_examples_workspace_bytes(1000, dim, 1, 10) == 0);
  for (int dim : {132, 256, 388, 768, 1000, 1536, 2052, 4096}) {
    for (int c : {1, 64, 65, 256, 257, 2048}) {
      size_t prev = 0;
      for (int64_t n : {int64_t{1}, int64_t{63}, int64_t{2053}, int64_t{1} << 20, (int64_t{1} << 32) - 1}) {
        const size_t got = dewi_knn_examples_workspace_bytes(n, dim, 4, c);
        EXPECT(got >= 8 * static_cast<size_t>(n) && got >= prev);
        EXPECT(got == dewi_knn_examples_workspace_bytes(n, dim, DEWI_EXAMPLES_MAX, c));
        if (c > 256) EXPECT(got >= 16 * static_cast<size_t>(n));     // dense keys: 8 more bytes per scanned row
        prev = got;
      }
    }
  }

  if (failures) {
    std::fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  std::puts("hostcheck_examples: ok");
  return 0;
}
