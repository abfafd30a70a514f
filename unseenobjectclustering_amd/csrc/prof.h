// Opt-in per-kernel-class timing with HIP events recorded on the launch stream.
// Off by default (zero overhead); bench.py switches it on for a dedicated profiled pass and
// reads the per-class launch count, total duration and algorithmic flops/bytes.
// Single-threaded use only.
#pragma once
#include <hip/hip_runtime.h>

namespace uoc {

enum KernelClass {
  KC_CONV_160x128 = 0,
  KC_CONV_80x128,
  KC_CONV_160x64,
  KC_CONV_80x64,
  KC_CONV_STEM,
  KC_GLDS_160x128,
  KC_GLDS_80x128,
  KC_GLDS_160x64,
  KC_GLDS_80x64,
  KC_WINO_INPUT,
  KC_WINO_GEMM,
  KC_NET_MISC,  // layout conversion, max-pool
  KC_HEAD,
  KC_FPS_STEP,
  KC_HC_ITER,
  KC_HC_FINALIZE,
  KC_SEED_CC,
  KC_ASSIGN,
  KC_RELABEL,
  KC_ROI,
  KC_WINO4_INPUT,
  KC_WINO4_GEMM,
  KC_WINO4_OUTPUT,
  KC_PLANE_CAND,     // support plane: candidate compaction
  KC_PLANE_HYP,      // hypothesis table
  KC_PLANE_SCORE,    // hypothesis scoring and the argmax
  KC_PLANE_REFINE,   // fp64 refinement over the winner's inliers
  KC_PLANE_OBJECTS,  // heights and upright boxes
  KC_REL_PAIRS,      // object relations: memsets and the pair tables
  KC_REL_DERIVE,     // relations, layers, order
  KC_PLACE_RASTER,     // placement: memsets and the top-down raster of the points
  KC_PLACE_TRANSFORM,  // cells, the distance transform and the queries
  KC_GRASP_MOMENTS,     // grasp candidates: the memset and the per-id moments
  KC_GRASP_CANDIDATES,  // the class table, the candidates and the best record
  KC_ELEV_RASTER,     // elevation map: memsets and the two point passes (top, near)
  KC_ELEV_TRANSFORM,  // cells, level, the distance transform, the per-id table and the queries
  KC_FOOT_TABLES,  // footprint fitting: memsets, the mask spans and the runs of free cells
  KC_FOOT_FIT,     // the fit words, the counts, the keys and the best records
  KC_ROUTES_TABLES,  // routes: the memset, the runs of free cells and the passable maps
  KC_ROUTES_SOLVE,   // the cost fields, the closest approach and the paths
  KC_MS_CONFIDENCE,  // label confidence: the assignment with the runner-up component and its margin
  KC_CONF_GLUE,      // the value paste along the paint plan and the per-id summary
  KC_NORMALS_PIXELS,  // surface normals: the memset and the per-pixel stencil with the face accumulators
  KC_NORMALS_FACES,   // the rows of the faces table
  KC_PLANES_CAND,     // multi-plane extraction: the memset and the first candidate compaction
  KC_PLANES_ROUNDS,   // per round: hypotheses, scoring, the argmax and the re-compaction of the survivors
  KC_PLANES_INDEX,    // the index map and the removed counts
  KC_PLANES_REFINE,   // fp64 refinement of every plane, the extents and the info records
  KC_PLANES_OBJECTS,  // heights and upright boxes against every plane
  KC_COUNT
};

// Optional launch-shape tag: the report also aggregates per (class, tag), so that one kernel class can be broken down
// by layer shape (convolutions: rows M of the GEMM, Cin, Cout, dilation).
struct ProfTag {
  int v[4] = {0, 0, 0, 0};
};

extern bool g_prof_enabled;
void prof_begin(int kc, hipStream_t st, double flops, double bytes, const ProfTag &tag);
void prof_end(hipStream_t st);

struct ProfScope {
  hipStream_t st;
  bool on;
  ProfScope(int kc, hipStream_t s, double flops, double bytes, const ProfTag &tag = ProfTag()) : st(s), on(g_prof_enabled) {
    if (on) prof_begin(kc, s, flops, bytes, tag);
  }
  ~ProfScope() {
    if (on) prof_end(st);
  }
};

}  // namespace uoc
