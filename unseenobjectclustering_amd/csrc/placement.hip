// Table occupancy and placement: free space on the support plane (include/uoc_hip.h, uoc_placement).
// From the label map, the XYZ planes and the uoc_plane record of a frame: a top-down grid of G x G cells in the plane's
// own axes (state, owner), the exact squared Euclidean distance of every cell to the nearest blocking cell (dist2) and
// the answers to up to 16 placement queries.  Integers only.
//
// Three memsets (the counters n_obs / n_table and the query keys in the workspace, d_owner, d_counts) and three
// launches, a fourth when there are queries:
//   raster_kernel   grid (pixel chunks of PIX_CHUNK, frames), 4 waves; a wave owns PIX_SUB consecutive pixels.  Every block
//                   turns the frame's plane record into the integer frame F (block 0 of a frame writes it out).  A lane
//                   owns 4 consecutive pixels per turn (one int4 and three float4 loads) when H*W is a multiple of 4 and
//                   the pointers are 16-byte aligned, else one pixel.  A point becomes at most two events: a count event
//                   (cell, table | obstacle) and, for a labelled obstacle, an owner event (cell, id).  The wave adds every
//                   DISTINCT event of its 256 (64) pixels once: ballot + popcount over the lanes and the four slots, then
//                   one integer atomicAdd / atomicMax to the counters in global memory (a 256^2 grid of three words per
//                   cell does not fit in LDS).  A wave whose lanes are all ignored touches nothing.
//   column_kernel   grid (strips of 32 columns, frames): state, owner, cells[]; then g[i][j] = the distance along i to the
//                   nearest blocking cell of column j, the virtual cells at i = -1 and i = G included: 8 row segments per
//                   column scanned up and down, the carry between segments through LDS.  g goes to d_dist2.
//   row_kernel      grid (rows, frames): dist2[i][j] = min over j' of (j-j')^2 + g[i][j']^2 with the virtual columns at
//                   -1 and G, the plain minimum over the row from LDS (every lane reads the same words: a broadcast), in
//                   place.  Per query one 64-bit key per candidate cell, the maximum per wave by shuffles, per block
//                   through LDS, per frame by atomicMax.
//   answer_kernel   one block per frame: the keys back into (i, j, dist2, ok).
//
// Determinism: integer adds and maxima commute; a minimum commutes; the query keys are strict total orders (the cell index
// is part of the key), so no result depends on the order in which lanes, waves or blocks arrive.  Nothing of frame b
// depends on the other frames of the batch.
//
// The frame and its record, step P, the pixel sweep, the merge of equal events (wave_distinct), the segment scan of the
// column pass, the row minimum and the widest key are grid.h's, shared with the other stages on this grid.
//
// The query keys and the answer are grid.h's too (rule Q), shared with scene.hip.
#include "grid.h"
#include "prof.h"

namespace uoc {
namespace {

constexpr int MAX_Q = PLACE_MAX_Q;
using Queries = PlaceQueries;

struct Thresholds {
  int cell_div;         // cell_mm * S
  int t_low, t_obs, t_tab;  // -tau_mm*S, h_obs_mm*S, tau_mm*S   (all below 2^24)
};

// One pixel after step P (grid.h): the count event (cell*2 + obstacle) and the owner event (cell*128 + id), -1 for none;
// returns true when the point lies outside the grid.
__device__ __forceinline__ bool classify(const Frame &f, const Thresholds &th, int G, int l, float x, float y, float z,
                                         int &e_cnt, int &e_own) {
  e_cnt = e_own = -1;
  return project_point(f, th.cell_div, th.t_low, G, x, y, z, [&](int i, int j, long long T) {
    const int id = obj_id(l);
    const int cell = i * G + j;
    if (id != 0 || T > th.t_obs) {
      e_cnt = cell * 2 + 1;
      if (id) e_own = cell * NUM_IDS + id;
    } else if (T <= th.t_tab) {
      e_cnt = cell * 2;
    }
  });
}

// ---- 1. raster --------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void raster_kernel(const int *__restrict__ labels, const float *__restrict__ xyz,
                                                     const uoc_plane *__restrict__ planes, long long n, int G,
                                                     Thresholds th, int *__restrict__ n_obs, int *__restrict__ n_table,
                                                     int *__restrict__ owner, int *__restrict__ counts,
                                                     long long *__restrict__ frame) {
  constexpr int K = VEC ? 4 : 1;
  const int tid = threadIdx.x, lane = tid & 63;
  const int c = blockIdx.x, b = blockIdx.y;
  const Frame f = frame_from_plane(planes[b]);
  if (c == 0 && tid == 0) store_frame(frame + (size_t)b * NFR, f);
  if (!f.found) return;  // uniform per frame
  const size_t cells = (size_t)G * G;
  int *NO = n_obs + (size_t)b * cells, *NT = n_table + (size_t)b * cells, *OW = owner + (size_t)b * cells;
  int outside = 0;
  Pixels<K> px;
  for (PixelSweep<VEC> sweep(labels + (size_t)b * n, xyz + (size_t)b * 3 * n, n); sweep.load(px);) {
    int e_cnt[K], e_own[K];
    const int none[K] = {};
    bool out[K];
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = classify(f, th, G, px.l[k], px.x[k], px.y[k], px.z[k], e_cnt[k], e_own[k]);
    outside += wave_count_set(out);
    wave_distinct<K, false>(e_cnt, none, lane, [&](int code, int total, int) { atomicAdd((code & 1) ? &NO[code >> 1] : &NT[code >> 1], total); });
    wave_distinct<K, false>(e_own, none, lane, [&](int code, int, int) { atomicMax(&OW[code >> 7], code & (NUM_IDS - 1)); });
  }
  if (lane == 0 && outside) atomicAdd(&counts[(size_t)b * NUM_IDS], outside);
}

// ---- 2. cells and the column pass ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(STRIP *SEGS) void column_kernel(const int *__restrict__ n_obs, const int *__restrict__ n_table,
                                                             const long long *__restrict__ frame, int G, int min_pts,
                                                             int unknown_blocks, int *__restrict__ state,
                                                             int *__restrict__ owner, int *__restrict__ g_out,
                                                             int *__restrict__ counts) {
  __shared__ unsigned short s[MAX_G][STRIP];  // bit 15: blocking; after the upward scan the low bits hold the distance up
  __shared__ int s_hist[NUM_IDS];
  const int tid = threadIdx.x, b = blockIdx.y, j0 = blockIdx.x * STRIP;
  const bool found = frame_found_nonzero(frame + (size_t)b * NFR);
  const size_t off = (size_t)b * G * G;
  if (tid < NUM_IDS) s_hist[tid] = 0;
  __syncthreads();
  for (int idx = tid; idx < G * STRIP; idx += STRIP * SEGS) {
    const int i = idx / STRIP, jj = idx % STRIP, j = j0 + jj;
    if (j >= G) continue;
    const size_t a = off + (size_t)i * G + j;
    int st = 0, ow = 0;
    if (found) {
      st = n_obs[a] >= min_pts ? 2 : (n_table[a] >= min_pts ? 1 : 0);
      ow = st == 2 ? owner[a] : 0;
      if (ow > 0) atomicAdd(&s_hist[ow], 1);
    }
    state[a] = st;
    owner[a] = ow;
    s[i][jj] = (!found || st == 2 || (st == 0 && unknown_blocks)) ? 0x8000u : 0u;
  }
  __syncthreads();
  if (tid >= 1 && tid < NUM_IDS && s_hist[tid]) atomicAdd(&counts[(size_t)b * NUM_IDS + tid], s_hist[tid]);
  column_scan(s, G, j0, g_out + off);
}

// ---- 3. the row pass and the queries -----------------------------------------------------------------------------------
__global__ __launch_bounds__(ROW_THREADS) void row_kernel(const int *__restrict__ state, int G, Queries qs, int Q,
                                                          int *__restrict__ dist2, unsigned long long *__restrict__ keys) {
  row_pass_and_keys(state, G, qs, Q, dist2, keys);
}

__global__ __launch_bounds__(64) void answer_kernel(const unsigned long long *__restrict__ keys, int G, Queries qs, int Q,
                                                    int *__restrict__ answers) {
  answer_queries(keys, G, qs, Q, answers);
}

bool shape_ok(int B, int H, int W, int G) { return image_ok(B, H, W) && grid_ok(G); }

struct Ws {
  int *n_obs, *n_table;        // [B][G][G] each
  unsigned long long *keys;    // [B][MAX_Q]
  size_t total;
};
Ws carve(void *base, int B, int G) {
  Ws w;
  char *p = (char *)base;
  const size_t grid = align_up((size_t)B * G * G * sizeof(int), 256);
  w.n_obs = (int *)p;
  w.n_table = (int *)(p ? p + grid : nullptr);
  w.keys = (unsigned long long *)(p ? p + 2 * grid : nullptr);
  w.total = 2 * grid + align_up((size_t)B * MAX_Q * sizeof(unsigned long long), 256);
  return w;
}

}  // namespace
}  // namespace uoc

using namespace uoc;

extern "C" {

size_t uoc_placement_workspace_bytes(int B, int H, int W, int G) {
  if (!shape_ok(B, H, W, G)) return 0;
  return carve(nullptr, B, G).total;
}

int uoc_placement(const int32_t *d_labels, const float *d_xyz, const uoc_plane *d_planes, int B, int H, int W, int G,
                  int cell_mm, int h_obs_mm, int tau_mm, int min_pts, int unknown_blocks, const int32_t *h_queries, int Q,
                  int32_t *d_state, int32_t *d_owner, int32_t *d_dist2, int32_t *d_counts, int64_t *d_frame,
                  int32_t *d_answers, void *d_ws, size_t ws_bytes, void *stream) {
  UOC_REQUIRE(d_labels && d_xyz && d_planes && d_state && d_owner && d_dist2 && d_counts && d_frame && d_ws,
              "uoc_placement: null labels / xyz / planes / state / owner / dist2 / counts / frame / workspace");
  UOC_REQUIRE(image_ok(B, H, W),
              "uoc_placement: bad shape B=%d H=%d W=%d (B in 1..65535, H*W below 2^31)", B, H, W);
  UOC_REQUIRE(grid_ok(G), "uoc_placement: grid = %d is not a multiple of 8 in [8, %d]", G, MAX_G);
  UOC_REQUIRE(cell_mm >= 1 && cell_mm <= 1000, "uoc_placement: cell_mm = %d outside [1, 1000]", cell_mm);
  UOC_REQUIRE(h_obs_mm >= 0 && h_obs_mm <= 1000, "uoc_placement: h_obs_mm = %d outside [0, 1000]", h_obs_mm);
  UOC_REQUIRE(tau_mm >= 1 && tau_mm <= 1000, "uoc_placement: tau_mm = %d outside [1, 1000]", tau_mm);
  UOC_REQUIRE(min_pts >= 1 && min_pts <= 65535, "uoc_placement: min_pts = %d outside [1, 65535]", min_pts);
  UOC_REQUIRE(unknown_blocks == 0 || unknown_blocks == 1, "uoc_placement: unknown_blocks = %d is neither 0 nor 1", unknown_blocks);
  Queries qs;
  if (const int rc = load_place_queries("uoc_placement", h_queries, d_answers, Q, qs)) return rc;
  const Ws w = carve(d_ws, B, G);
  UOC_REQUIRE(ws_bytes >= w.total, "uoc_placement: workspace %zu < %zu bytes", ws_bytes, w.total);
  UOC_REQUIRE(aligned16(d_ws), "uoc_placement: workspace not 16-byte aligned");
  const long long n = (long long)H * W;
  const int nch = (int)((n + PIX_CHUNK - 1) / PIX_CHUNK);
  const size_t cells = (size_t)B * G * G;
  const Thresholds th = {cell_mm * SCALE, -tau_mm * SCALE, h_obs_mm * SCALE, tau_mm * SCALE};
  const bool vec = n % 4 == 0 && (((uintptr_t)d_labels | (uintptr_t)d_xyz) & 15) == 0;
  hipStream_t st = (hipStream_t)stream;
  {
    ProfScope prof(KC_PLACE_RASTER, st, 0.0, (double)B * n * 16.0 + (double)cells * 12.0);
    UOC_HIP_CHECK(hipMemsetAsync(d_ws, 0, w.total, st));
    UOC_HIP_CHECK(hipMemsetAsync(d_owner, 0, cells * sizeof(int32_t), st));
    UOC_HIP_CHECK(hipMemsetAsync(d_counts, 0, (size_t)B * NUM_IDS * sizeof(int32_t), st));
    if (vec)
      hipLaunchKernelGGL(raster_kernel<true>, dim3(nch, B), dim3(256), 0, st, d_labels, d_xyz, d_planes, n, G, th, w.n_obs,
                         w.n_table, d_owner, d_counts, (long long *)d_frame);
    else
      hipLaunchKernelGGL(raster_kernel<false>, dim3(nch, B), dim3(256), 0, st, d_labels, d_xyz, d_planes, n, G, th, w.n_obs,
                         w.n_table, d_owner, d_counts, (long long *)d_frame);
  }
  {
    ProfScope prof(KC_PLACE_TRANSFORM, st, (double)cells * G * 3.0, (double)cells * 28.0);
    hipLaunchKernelGGL(column_kernel, dim3((G + STRIP - 1) / STRIP, B), dim3(STRIP * SEGS), 0, st, w.n_obs, w.n_table,
                       (const long long *)d_frame, G, min_pts, unknown_blocks, d_state, d_owner, d_dist2, d_counts);
    hipLaunchKernelGGL(row_kernel, dim3(G, B), dim3(ROW_THREADS), 0, st, d_state, G, qs, Q, d_dist2, w.keys);
    if (Q > 0) hipLaunchKernelGGL(answer_kernel, dim3(B), dim3(64), 0, st, w.keys, G, qs, Q, d_answers);
  }
  UOC_LAUNCH_CHECK();
  return UOC_OK;
}

}  // extern "C"
