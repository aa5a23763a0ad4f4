// Host check of dewi_predicate_masks: the validation of its arguments and programs, which abi.cpp does before any device
// work.  Every array is exactly as long as the call says, so that a read past a program, a length or a column table shows
// under the host sanitizers.  A program of its own that needs no GPU:  make hostcheck  (csrc/Makefile) builds and runs it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

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

static int run(const std::vector<std::vector<dewi_pred_instr>>& programs, int n_columns, const std::vector<int32_t>& types,
               int64_t n_rows, int64_t n_set_words) {
  std::vector<dewi_pred_instr> flat;
  std::vector<int32_t> lengths;
  for (const auto& p : programs) {
    flat.insert(flat.end(), p.begin(), p.end());
    lengths.push_back(static_cast<int32_t>(p.size()));
  }
  if (flat.empty()) flat.push_back(dewi_pred_instr{DEWI_PRED_TRUE, 0, 0, 0});
  std::vector<const void*> cols(static_cast<size_t>(n_columns > 0 ? n_columns : 0), dummy);
  return dewi_predicate_masks(cols.empty() ? nullptr : cols.data(), types.empty() ? nullptr : types.data(), n_columns, n_rows,
                              flat.data(), lengths.data(), static_cast<int>(programs.size()),
                              n_set_words > 0 ? reinterpret_cast<const uint32_t*>(dummy) : nullptr, n_set_words, nullptr, dummy,
                              nullptr);
}

int main() {
  const dewi_pred_instr T{DEWI_PRED_TRUE, 0, 0, 0}, A{DEWI_PRED_AND, 0, 0, 0}, O{DEWI_PRED_OR, 0, 0, 0}, N{DEWI_PRED_NOT, 0, 0, 0};
  const std::vector<int32_t> types = {0, 1};
  // valid programs of every length and of the deepest stack, with n_rows == 0: validated in full, nothing launched
  for (int len = 1; len <= DEWI_PRED_MAX_INSTR; ++len) {
    std::vector<dewi_pred_instr> p;
    const int pushes = (len + 1) / 2;                       // pushes leaves, folds them, pads with NOTs
    for (int i = 0; i < pushes; ++i) p.push_back(i % 2 ? dewi_pred_instr{DEWI_PRED_F_LT, 1, 0, 0} : dewi_pred_instr{DEWI_PRED_I_GE, 0, 5, 0});
    for (int i = 0; i < pushes - 1; ++i) p.push_back(i % 2 ? A : O);
    while (static_cast<int>(p.size()) < len) p.push_back(N);
    EXPECT(static_cast<int>(p.size()) == len);
    EXPECT(run({p}, 2, types, 0, 0) == DEWI_OK);
    EXPECT(run({p, p, {T}}, 2, types, 0, 0) == DEWI_OK);
  }
  EXPECT(run(std::vector<std::vector<dewi_pred_instr>>(DEWI_PRED_MAX_PROGRAMS, {T}), 0, {}, 0, 0) == DEWI_OK);
  EXPECT(run({{{DEWI_PRED_I_IN_SET, 0, 3, 32}}}, 2, types, 0, 4) == DEWI_OK);
  // refusals
  EXPECT(run({{{DEWI_PRED_I_IN_SET, 0, 3, 33}}}, 2, types, 0, 4) == DEWI_ERR_INVALID_ARG);
  EXPECT(run({{{DEWI_PRED_I_IN_SET, 0, 0xFFFFFFFFu, 0xFFFFFFFFu}}}, 2, types, 0, 4) == DEWI_ERR_INVALID_ARG);
  EXPECT(run({{{DEWI_PRED_I_LT, 2, 0, 0}}}, 2, types, 0, 0) == DEWI_ERR_INVALID_ARG);
  EXPECT(run({{{DEWI_PRED_I_LT, -1, 0, 0}}}, 2, types, 0, 0) == DEWI_ERR_INVALID_ARG);
  EXPECT(run({{{DEWI_PRED_I_LT, 1, 0, 0}}}, 2, types, 0, 0) == DEWI_ERR_INVALID_ARG);
  EXPECT(run({{{DEWI_PRED_F_IS_NAN, 0, 0, 0}}}, 2, types, 0, 0) == DEWI_ERR_INVALID_ARG);
  EXPECT(run({{{22, 0, 0, 0}}}, 2, types, 0, 0) == DEWI_ERR_INVALID_ARG);
  EXPECT(run({{{-1, 0, 0, 0}}}, 2, types, 0, 0) == DEWI_ERR_INVALID_ARG);
  EXPECT(run({{T, A}}, 2, types, 0, 0) == DEWI_ERR_INVALID_ARG);
  EXPECT(run({{N}}, 2, types, 0, 0) == DEWI_ERR_INVALID_ARG);
  EXPECT(run({{T, T}}, 2, types, 0, 0) == DEWI_ERR_INVALID_ARG);
  EXPECT(run({std::vector<dewi_pred_instr>(65, T)}, 2, types, 0, 0) == DEWI_ERR_INVALID_ARG);
  {
    std::vector<dewi_pred_instr> deep(33, T);
    deep.insert(deep.end(), 31, A);
    EXPECT(run({deep}, 2, types, 0, 0) == DEWI_ERR_INVALID_ARG);
  }
  EXPECT(run({{T}}, 2, {0, 2}, 0, 0) == DEWI_ERR_INVALID_ARG);
  EXPECT(run({{T}}, 2, types, -1, 0) == DEWI_ERR_INVALID_ARG);
  EXPECT(run({{T}}, 2, types, int64_t{1} << 32, 0) == DEWI_ERR_UNSUPPORTED);
  EXPECT(run({{T}}, 17, std::vector<int32_t>(17, 0), 0, 0) == DEWI_ERR_UNSUPPORTED);
  EXPECT(run(std::vector<std::vector<dewi_pred_instr>>(DEWI_PRED_MAX_PROGRAMS + 1, {T}), 0, {}, 0, 0) == DEWI_ERR_UNSUPPORTED);
  EXPECT(run({}, 2, types, 0, 0) == DEWI_ERR_INVALID_ARG);
  EXPECT(dewi_predicate_masks(nullptr, nullptr, 0, 0, nullptr, nullptr, 1, nullptr, 0, nullptr, dummy, nullptr) == DEWI_ERR_INVALID_ARG);

  if (failures) {
    std::fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  std::puts("hostcheck_where: ok");
  return 0;
}
