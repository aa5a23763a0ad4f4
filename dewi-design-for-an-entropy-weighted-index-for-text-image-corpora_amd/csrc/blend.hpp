// The DEWI blend of step 4 (reference backends.py:461-465), shared by the select / re-rank kernels (select_rerank.hip) and the
// range collect (range.hip): one definition, so that a range result's adjusted score is the search's bit for bit.
#pragma once
#include "common.hpp"
#include "launch.hpp"

namespace dewi {

__device__ __forceinline__ float blend(const RerankParams& rp, float sim, float dewi, float ent) {
  // A10: the reference's HNSW / FAISS backends blend a similarity derived from the library's distance
  // (backends.py:229-231 `1 - dist`; :338-341 `1.0 / (1.0 + dist)`), not the raw score.  The library's
  // distance is 1 - <e,q> (hnswlib cosine, fp32) or the squared L2 distance (= -score in l2 space).
  if (rp.transform != DEWI_SIM_RAW) {
    const float dist = rp.space == DEWI_SPACE_L2 ? -sim : __fsub_rn(1.f, sim);
    sim = rp.transform == DEWI_SIM_ONE_MINUS_DIST ? __fsub_rn(1.f, dist) : __fdiv_rn(1.f, __fadd_rn(1.f, dist));
  }
  // reference backends.py:461-465: (1-eta)*s and eta*dewi are rounded separately, then added.
  float adj = __fadd_rn(__fmul_rn(rp.w_sim, sim), __fmul_rn(rp.w_dewi, dewi));
  if (rp.use_ent) adj = __fadd_rn(adj, __fmul_rn(rp.w_ent, ent));
  return adj;
}

}  // namespace dewi
