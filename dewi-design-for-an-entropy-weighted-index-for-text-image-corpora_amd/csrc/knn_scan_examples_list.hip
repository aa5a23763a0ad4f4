// Search by examples, the LIST form (the rows of one prepared allow-list): see scan_examples.hpp.
//
// Roofline: HBM.  Algorithmic bytes per pass = n_allowed * (dim * 4 + 4) (+ 8 * n_allowed per chained pass) + n_examples * dim * 4.
#include "scan_examples.hpp"

namespace dewi {

hipError_t launch_scan_examples_list(const ScanPlan& plan, const float* d_E, const float* d_X, const ExamplesPass& ps, int ne,
                                     float* part_p, float* part_n, const int64_t* d_exclude, const uint32_t* d_filter, int c,
                                     uint64_t* keys, hipStream_t stream) {
  return launch_scan_examples_impl<true>(plan, d_E, 0, d_X, ps, ne, part_p, part_n, d_exclude, d_filter, c, keys, stream);
}

}  // namespace dewi
