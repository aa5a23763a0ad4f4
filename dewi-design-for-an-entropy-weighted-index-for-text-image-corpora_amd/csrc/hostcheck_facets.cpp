// Host check of the facet entry points (include/dewi_hip.h "FACETS"): every argument error of dewi_facet_run in the stated
// order, the limits at and one past each bound, the size and plan functions, the tuning switch.  All of that runs before any
// device work, so this program needs no GPU:  make hostcheck  (csrc/Makefile) builds and runs it under the host sanitizers.
//
// n_rows == 0 is the one valid call made here.  Its contract is DEWI_OK with CLEARED outputs, which is device work; without
// a device the launch itself fails, so the check is that the call gets past every argument check: DEWI_OK or DEWI_ERR_HIP,
// nothing else.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../../include/dewi_hip.h"

static int failures = 0;

#define EXPECT(cond)                                          \
  do {                                                        \
    if (!(cond)) {                                            \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
      ++failures;                                             \
    }                                                         \
  } while (0)

alignas(16) static unsigned char dummy[64];   // stands for device memory: nobody reads it, no refused call reaches the device

struct Call {
  const void* keys = dummy;
  int key_kind = DEWI_FACET_KEY_I32_RANGE;
  int64_t n_rows = 10;
  int32_t key_lo = 0;
  const void* edges = nullptr;
  int64_t n_bins = 4;
  int sel_kind = DEWI_FACET_SEL_ALL;
  int p = 1;
  const uint8_t* masks = nullptr;
  const int64_t* rows = nullptr;
  const int64_t* lims = nullptr;
  int64_t n_listed = 0;
  const void* values = nullptr;
  int value_type = DEWI_FACET_VALUE_NONE;
  int64_t* counts = reinterpret_cast<int64_t*>(dummy);
  int64_t* vcount = nullptr;
  void* vmin = nullptr;
  void* vmax = nullptr;
  void* vsum = nullptr;
  void* ws = dummy;
  long long ws_bytes = -1;   // -1: what the size function asks for

  Call& masks_of(int n) {
    sel_kind = DEWI_FACET_SEL_MASKS, p = n, masks = dummy;
    return *this;
  }
  Call& lists_of(int n, int64_t t) {
    sel_kind = DEWI_FACET_SEL_LISTS, p = n, n_listed = t, rows = reinterpret_cast<const int64_t*>(dummy),
    lims = reinterpret_cast<const int64_t*>(dummy);
    return *this;
  }
  Call& with_values(int type) {
    value_type = type, values = dummy, vcount = reinterpret_cast<int64_t*>(dummy), vmin = vmax = vsum = dummy;
    return *this;
  }
  int run() const {
    size_t bytes = ws_bytes >= 0 ? static_cast<size_t>(ws_bytes) : dewi_facet_workspace_bytes(n_bins, p, value_type);
    if (ws_bytes < 0 && bytes == 0) bytes = 256;
    return dewi_facet_run(keys, key_kind, n_rows, key_lo, edges, n_bins, sel_kind, p, masks, rows, lims, n_listed, values, value_type,
                          counts, vcount, vmin, vmax, vsum, ws, bytes, nullptr);
  }
};

static bool last_error_has(const char* word) { return std::strstr(dewi_last_error(), word) != nullptr; }

int main() {
  const int inv = DEWI_ERR_INVALID_ARG, uns = DEWI_ERR_UNSUPPORTED, wsp = DEWI_ERR_WORKSPACE;
  // 1. enums — before a null pointer is looked at
  { Call c; c.key_kind = 3; c.keys = nullptr; EXPECT(c.run() == inv && last_error_has("key_kind")); }
  { Call c; c.key_kind = -1; EXPECT(c.run() == inv && last_error_has("key_kind")); }
  { Call c; c.sel_kind = 3; c.keys = nullptr; EXPECT(c.run() == inv && last_error_has("sel_kind")); }
  { Call c; c.sel_kind = -1; EXPECT(c.run() == inv && last_error_has("sel_kind")); }
  { Call c; c.value_type = 3; c.keys = nullptr; EXPECT(c.run() == inv && last_error_has("value_type")); }
  { Call c; c.value_type = -1; EXPECT(c.run() == inv && last_error_has("value_type")); }
  // 2. pointers — before the sizes (n_rows = -1 in every call)
  { Call c; c.n_rows = -1; c.keys = nullptr; EXPECT(c.run() == inv && last_error_has("null pointer")); }
  { Call c; c.n_rows = -1; c.counts = nullptr; EXPECT(c.run() == inv && last_error_has("null pointer")); }
  { Call c; c.n_rows = -1; c.key_kind = DEWI_FACET_KEY_I32_EDGES; EXPECT(c.run() == inv && last_error_has("null pointer")); }
  { Call c; c.n_rows = -1; c.key_kind = DEWI_FACET_KEY_F32_EDGES; EXPECT(c.run() == inv && last_error_has("null pointer")); }
  { Call c; c.n_rows = -1; c.masks_of(2).masks = nullptr; EXPECT(c.run() == inv && last_error_has("null pointer")); }
  { Call c; c.n_rows = -1; c.lists_of(2, 5).rows = nullptr; EXPECT(c.run() == inv && last_error_has("null pointer")); }
  { Call c; c.n_rows = -1; c.lists_of(2, 5).lims = nullptr; EXPECT(c.run() == inv && last_error_has("null pointer")); }
  { Call c; c.n_rows = -1; c.with_values(DEWI_FACET_VALUE_I32).values = nullptr; EXPECT(c.run() == inv && last_error_has("null pointer")); }
  { Call c; c.n_rows = -1; c.with_values(DEWI_FACET_VALUE_F32).vcount = nullptr; EXPECT(c.run() == inv && last_error_has("null pointer")); }
  { Call c; c.n_rows = -1; c.with_values(DEWI_FACET_VALUE_F32).vmin = nullptr; EXPECT(c.run() == inv && last_error_has("null pointer")); }
  { Call c; c.n_rows = -1; c.with_values(DEWI_FACET_VALUE_F32).vmax = nullptr; EXPECT(c.run() == inv && last_error_has("null pointer")); }
  { Call c; c.n_rows = -1; c.with_values(DEWI_FACET_VALUE_I32).vsum = nullptr; EXPECT(c.run() == inv && last_error_has("null pointer")); }
  // 3. sizes — before the limits (n_rows = 2^32 elsewhere in the call)
  { Call c; c.n_rows = -1; c.n_bins = DEWI_FACET_MAX_BINS + 1; EXPECT(c.run() == inv); }
  { Call c; c.n_rows = int64_t{1} << 32; c.n_bins = 0; EXPECT(c.run() == inv); }
  { Call c; c.n_rows = int64_t{1} << 32; c.masks_of(0); EXPECT(c.run() == inv); }
  { Call c; c.n_rows = int64_t{1} << 32; c.lists_of(1, -1); EXPECT(c.run() == inv); }
  { Call c; c.n_rows = int64_t{1} << 32; c.p = 2; EXPECT(c.run() == inv && last_error_has("SEL_ALL")); }
  // 4. limits, one past each bound — before the workspace (0 bytes)
  { Call c; c.ws_bytes = 0; c.n_bins = DEWI_FACET_MAX_BINS + 1; EXPECT(c.run() == uns); }
  { Call c; c.ws_bytes = 0; c.masks_of(DEWI_FACET_MAX_SELECTIONS + 1); EXPECT(c.run() == uns); }
  { Call c; c.ws_bytes = 0; c.masks_of(128).n_bins = DEWI_FACET_MAX_BINS; EXPECT(c.run() == uns && last_error_has("MAX_SLOTS")); }
  { Call c; c.ws_bytes = 0; c.masks_of(DEWI_FACET_MAX_SELECTIONS).n_bins = (1 << 15) - 1; EXPECT(c.run() == uns && last_error_has("MAX_SLOTS")); }
  { Call c; c.ws_bytes = 0; c.n_rows = int64_t{1} << 32; EXPECT(c.run() == uns); }
  { Call c; c.ws_bytes = 0; c.lists_of(1, int64_t{1} << 32); EXPECT(c.run() == uns); }
  // ... and AT each bound the call gets as far as the workspace check
  { Call c; c.ws_bytes = 0; c.n_bins = DEWI_FACET_MAX_BINS; EXPECT(c.run() == wsp); }
  { Call c; c.ws_bytes = 0; c.masks_of(DEWI_FACET_MAX_SELECTIONS); EXPECT(c.run() == wsp); }
  { Call c; c.ws_bytes = 0; c.masks_of(127).n_bins = DEWI_FACET_MAX_BINS; EXPECT(c.run() == wsp); }
  { Call c; c.ws_bytes = 0; c.masks_of(DEWI_FACET_MAX_SELECTIONS).n_bins = (1 << 15) - 2; EXPECT(c.run() == wsp); }   // exactly 2^27 slots
  { Call c; c.ws_bytes = 0; c.n_rows = (int64_t{1} << 32) - 1; EXPECT(c.run() == wsp); }
  { Call c; c.ws_bytes = 0; c.lists_of(1, (int64_t{1} << 32) - 1); EXPECT(c.run() == wsp); }
  // 5. the workspace: one byte short, and a null one
  { Call c; c.ws_bytes = 255; EXPECT(c.run() == wsp); }
  { Call c; c.ws = nullptr; EXPECT(c.run() == wsp); }
  {
    Call c;
    c.masks_of(5).with_values(DEWI_FACET_VALUE_F32).n_bins = 1000;
    const size_t need = dewi_facet_workspace_bytes(1000, 5, DEWI_FACET_VALUE_F32);
    EXPECT(need == ((size_t{2} * 4 * 5 * 1002 + 255) / 256) * 256);
    c.ws_bytes = static_cast<long long>(need) - 1;
    EXPECT(c.run() == wsp);
  }
  // n_rows == 0 and an empty list: past every argument check (see the head of this file)
  { Call c; c.n_rows = 0; const int rc = c.run(); EXPECT(rc == DEWI_OK || rc == DEWI_ERR_HIP); }
  { Call c; c.lists_of(3, 0); const int rc = c.run(); EXPECT(rc == DEWI_OK || rc == DEWI_ERR_HIP); }
  { Call c; c.n_rows = 0; c.masks_of(3).with_values(DEWI_FACET_VALUE_I32); const int rc = c.run(); EXPECT(rc == DEWI_OK || rc == DEWI_ERR_HIP); }

  // the size function: 0 for what the call refuses, never 0 otherwise
  EXPECT(dewi_facet_workspace_bytes(4, 1, DEWI_FACET_VALUE_NONE) == 256);
  EXPECT(dewi_facet_workspace_bytes(0, 1, DEWI_FACET_VALUE_NONE) == 0);
  EXPECT(dewi_facet_workspace_bytes(DEWI_FACET_MAX_BINS + 1, 1, DEWI_FACET_VALUE_NONE) == 0);
  EXPECT(dewi_facet_workspace_bytes(4, 0, DEWI_FACET_VALUE_NONE) == 0);
  EXPECT(dewi_facet_workspace_bytes(4, DEWI_FACET_MAX_SELECTIONS + 1, DEWI_FACET_VALUE_NONE) == 0);
  EXPECT(dewi_facet_workspace_bytes(DEWI_FACET_MAX_BINS, 128, DEWI_FACET_VALUE_NONE) == 0);
  EXPECT(dewi_facet_workspace_bytes(4, 1, 3) == 0);
  EXPECT(dewi_facet_workspace_bytes(DEWI_FACET_MAX_BINS, 127, DEWI_FACET_VALUE_F32) == ((size_t{8} * 127 * (DEWI_FACET_MAX_BINS + 2) + 255) / 256) * 256);

  // the plan: path 0 while one selection's counters fit DEWI_FACET_LDS_COUNTER_BYTES; never more than 64 KB of LDS
  int64_t w[DEWI_FACET_PLAN_WORDS];
  EXPECT(dewi_facet_tuning_set(-1, 0) == DEWI_OK);
  EXPECT(dewi_facet_plan(1000, 0, DEWI_FACET_LDS_COUNTER_BYTES / 4 - 2, 0, 1, 0, w) == DEWI_OK && w[0] == 0 && w[3] == DEWI_FACET_LDS_COUNTER_BYTES);
  EXPECT(dewi_facet_plan(1000, 0, DEWI_FACET_LDS_COUNTER_BYTES / 4 - 1, 0, 1, 0, w) == DEWI_OK && w[0] == 1 && w[3] == 0);
  EXPECT(dewi_facet_plan(1000, 0, DEWI_FACET_LDS_COUNTER_BYTES / 24 - 2, 1, 7, 2, w) == DEWI_OK && w[0] == 0 && w[2] == 1 && w[4] == 7);
  EXPECT(dewi_facet_plan(1000, 0, DEWI_FACET_LDS_COUNTER_BYTES / 24 - 1, 1, 7, 1, w) == DEWI_OK && w[0] == 1 && w[2] == 7 && w[4] == 1);
  for (int kind = 0; kind < 3; ++kind)
    for (int vt = 0; vt < 3; ++vt)
      for (int64_t bins : {int64_t{1}, int64_t{2046}, int64_t{4095}, int64_t{4096}, int64_t{12286}, int64_t{DEWI_FACET_MAX_BINS}})
        EXPECT(dewi_facet_plan(5000, kind, bins, 1, 3, vt, w) == DEWI_OK && w[3] >= 0 && w[3] <= 65536 && w[1] >= 1 && w[2] >= 1 && w[2] * w[4] >= 3);
  EXPECT(dewi_facet_plan(1 << 20, 0, 1000, 1, 33, 0, w) == DEWI_OK && w[0] == 0 && w[2] == 12 && w[4] == 3 && w[1] == 256);
  EXPECT(dewi_facet_plan(5000, 0, 1000, 2, 12, 0, w) == DEWI_OK && w[0] == 0);
  EXPECT(dewi_facet_plan(5000, 0, 1000, 2, 13, 0, w) == DEWI_OK && w[0] == 1);
  EXPECT(dewi_facet_tuning_set(1, 3) == DEWI_OK);
  EXPECT(dewi_facet_plan(1 << 20, 0, 1000, 1, 33, 0, w) == DEWI_OK && w[0] == 1 && w[1] == 3 && w[2] == 33 && w[4] == 1);
  EXPECT(dewi_facet_tuning_set(-1, 0) == DEWI_OK);
  EXPECT(dewi_facet_plan(int64_t{1} << 32, 0, 4, 0, 1, 0, w) == uns);
  EXPECT(dewi_facet_plan((int64_t{1} << 32) - 1, 0, 4, 0, 1, 0, w) == DEWI_OK && w[1] == 512);
  EXPECT(dewi_facet_plan(10, 0, 4, 0, 1, 0, nullptr) == inv);
  EXPECT(dewi_facet_plan(10, 3, 4, 0, 1, 0, w) == inv);
  EXPECT(dewi_facet_plan(10, 0, 4, 0, 2, 0, w) == inv);

  if (failures) {
    std::fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  std::puts("hostcheck_facets: ok");
  return 0;
}
