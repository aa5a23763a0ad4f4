// Search by examples, the dense form (every row of the corpus) and the plan: see scan_examples.hpp.
//
// Roofline: HBM.  Algorithmic bytes per pass = n_rows * dim * 4 (+ 8 * n_rows per chained pass) + n_examples * dim * 4.
#include "scan_examples.hpp"

namespace dewi {

// The geometry of scan_rows_any for rows of whole units (plan_scan's rules: slots for c <= 64, c <= 256, dense above; one
// 8-wave workgroup per compute unit, never more waves than give each at least four steps of work) on a fixed number of
// compute units, so that the workspace size needs no device.  nq_max: the examples one pass holds.  kind == kScanGeneric:
// a shape the route does not take.
ScanPlan plan_scan_examples(int64_t n_scan, int dim, int n_candidates) {
  ScanPlan p{};
  p.kind = kScanGeneric;
  if (n_scan <= 0 || dim <= 0 || dim % 4 != 0 || n_candidates <= 0) return p;
  const int units = dim / 4;
  if (units <= 32 || units > 64 * 16) return p;
  static const int pads[] = {1, 2, 3, 4, 5, 6, 8, 10, 12, 16};
  const int need = (units + 63) / 64;
  for (int v : pads)
    if (v >= need) { p.u_pad = v; break; }
  p.kind = kScanAnyLong;
  p.units = units;
  p.vec = 4;
  p.group = kWave;
  p.row_cols = dim;
  p.level = any_level(units);
  p.rows_per_iter = p.rows_per_iter_batch = any_rows(p.u_pad, 1, p.level);
  p.nq_max = any_nq_max(4, p.u_pad);
  p.nq_per_launch = p.nq_max;
  p.raw_queries = true;
  p.nontemporal = true;
  p.dense = n_candidates > kMaxListCandidates;
  const int64_t groups = (n_scan + p.rows_per_iter - 1) / p.rows_per_iter;
  int64_t blocks = (groups + 4 * (kScanThreads / kWave) - 1) / (4 * (kScanThreads / kWave));
  if (blocks < 1) blocks = 1;
  if (blocks > kExamplesMaxBlocks) blocks = kExamplesMaxBlocks;
  p.blocks = static_cast<int>(blocks);
  p.waves = p.blocks * (kScanThreads / kWave);
  p.slots = p.dense ? 0 : (n_candidates <= kWave ? 1 : kMaxSlots);
  p.n_lists = p.dense ? 0 : (p.slots == 1 ? p.blocks : p.waves);
  p.keys_per_query = p.dense ? n_scan : static_cast<int64_t>(p.n_lists) * n_candidates;
  return p;
}

hipError_t launch_scan_examples(const ScanPlan& plan, const float* d_E, int64_t n_rows, const float* d_X, const ExamplesPass& ps,
                                int ne, float* part_p, float* part_n, const int64_t* d_exclude, int c, uint64_t* keys,
                                hipStream_t stream) {
  return launch_scan_examples_impl<false>(plan, d_E, n_rows, d_X, ps, ne, part_p, part_n, d_exclude, nullptr, c, keys, stream);
}

}  // namespace dewi
