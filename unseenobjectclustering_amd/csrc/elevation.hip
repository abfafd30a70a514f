// Elevation map: object tops and stacking spots on the table grid (include/uoc_hip.h, uoc_elevation).
// From the label map, the XYZ planes and the integer frame record of uoc_placement: per cell of the same G x G grid the
// height of the highest point above the plane (elev), its id (owner), the point counts (pts, near), the exact squared
// Euclidean distance to the nearest cell that is not level (dist2), a per-id table of tops and the answers to up to 16
// queries.  Integers only.
//
// Four memsets (the top words and the accumulators in the workspace, d_pts, d_near, d_info) and five launches:
//   point_kernel<.., 1>  grid (pixel chunks of PIX_CHUNK, frames), 4 waves; a wave owns PIX_SUB consecutive pixels.  A lane owns 4
//                   consecutive pixels per turn (one int4 and three float4 loads) when H*W is a multiple of 4 and the
//                   pointers are 16-byte aligned, else one pixel.  A kept point is (cell, word), word = (key << 7) | id.
//                   Per DISTINCT cell of the wave's 256 (64) pixels: ballot + popcount for the count, shuffles for the
//                   maximum word, then one atomicAdd to pts and one atomicMax to top.
//   point_kernel<.., 2>  the same traversal; top is complete (kernel boundary).  A point with key >= (top >> 7) - step_mm
//                   is a near point; one atomicAdd of the combined count per distinct cell.
//   cell_kernel     grid (strips of 32 columns, frames): elev, owner, solid and blocking from the four edge neighbours
//                   (their words come from global memory: the strip with its halo at G = 512 does not fit in LDS), the
//                   counters of info; then g[i][j] = the distance along i to the nearest blocking cell of column j, the
//                   virtual cells at i = -1 and i = G included: 8 row segments per column scanned up and down, the carry
//                   between segments through LDS.  g goes to d_dist2.
//   row_kernel      grid (rows, frames): dist2[i][j] = min over j' of (j-j')^2 + g[i][j']^2 with the virtual columns at
//                   -1 and G, the plain minimum over the row from LDS, in place.  Per id the counts, the key of the widest
//                   level cell, the largest elev and the sum of elev: combined per wave over its distinct owners (ballot
//                   and shuffles), per block in LDS, per frame by integer atomics; per query one 64-bit key per candidate,
//                   the maximum per wave by shuffles, per block through LDS, per frame by atomicMax.
//   answer_kernel   one block per frame: the accumulators into the rows of tops, the keys into answers.
//
// Determinism: integer adds and maxima commute; a minimum commutes; the keys are strict total orders (the cell index is
// part of the key), so no result depends on the order in which lanes, waves or blocks arrive.  Nothing of frame b
// depends on the other frames of the batch.
//
// The frame record, step P, the pixel sweep, the merge of equal cells (wave_distinct), the segment scan of the column
// pass, the row minimum and the widest key are grid.h's: the definitions placement.hip uses.
//
// Key of "widest" (0: no candidate).  dist2 <= (G/2)^2 = 2^16, idx = i*G + j < 2^18:
//   ((dist2 + 1) << 18) | (0x3FFFF - idx)
#include "grid.h"
#include "prof.h"

namespace uoc {
namespace {

constexpr int MAX_Q = UOC_ELEV_MAX_QUERIES;
constexpr int KEY_BIAS = 1024;      // key = hq + 1024 >= 24: a word of 0 means "no point"
constexpr int HQ_MAX = 32767;

static_assert(((HQ_MAX + KEY_BIAS) << 7 | (NUM_IDS - 1)) > 0, "a word is a positive int");

struct Queries {
  int v[MAX_Q][4];  // need2, id, hmin_mm, hmax_mm
};

// One pixel after step P (grid.h): cell (-1: not kept) and word; returns true when the point lies outside the grid.
__device__ __forceinline__ bool project(const Frame &f, int cell_div, int t_low, int G, int l, float x, float y, float z,
                                        int &cell, int &word) {
  cell = -1;
  word = 0;
  return project_point(f, cell_div, t_low, G, x, y, z, [&](int i, int j, long long T) {
    const long long hq = min(T >> 14, (long long)HQ_MAX);  // arithmetic shift: a floor; hq >= -tau_mm >= -1000
    cell = i * G + j;
    word = (((int)hq + KEY_BIAS) << 7) | obj_id(l);
  });
}

// ---- 1, 2. the point passes ---------------------------------------------------------------------------------------------
template <bool VEC, int PASS>
__global__ __launch_bounds__(256) void point_kernel(const int *__restrict__ labels, const float *__restrict__ xyz,
                                                    const long long *__restrict__ frame, long long n, int G, int cell_div,
                                                    int t_low, int step_mm, int *__restrict__ top, int *__restrict__ pts,
                                                    int *__restrict__ near, int *__restrict__ info) {
  constexpr int K = VEC ? 4 : 1;
  const int lane = threadIdx.x & 63, b = blockIdx.y;
  const Frame f = load_frame(frame + (size_t)b * NFR);
  if (!f.found) return;  // uniform per frame
  const size_t cells = (size_t)G * G;
  int *TOP = top + (size_t)b * cells, *PTS = pts + (size_t)b * cells, *NEAR = near + (size_t)b * cells;
  int outside = 0;
  Pixels<K> px;
  for (PixelSweep<VEC> sweep(labels + (size_t)b * n, xyz + (size_t)b * 3 * n, n); sweep.load(px);) {
    int e[K], wd[K];
    bool out[K];
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = project(f, cell_div, t_low, G, px.l[k], px.x[k], px.y[k], px.z[k], e[k], wd[k]);
    if constexpr (PASS == 1) {
      outside += wave_count_set(out);
      wave_distinct<K, true>(e, wd, lane, [&](int cell, int total, int word) {
        atomicAdd(&PTS[cell], total);
        atomicMax(&TOP[cell], word);
      });
    } else {
#pragma unroll
      for (int k = 0; k < K; ++k)
        if (e[k] >= 0 && (wd[k] >> 7) < (TOP[e[k]] >> 7) - step_mm) e[k] = -1;
      wave_distinct<K, false>(e, wd, lane, [&](int cell, int total, int) { atomicAdd(&NEAR[cell], total); });
    }
  }
  if (PASS == 1 && lane == 0 && outside) atomicAdd(&info[(size_t)b * 4 + 1], outside);
}

// ---- 3. cells and the column pass ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(STRIP *SEGS) void cell_kernel(const int *__restrict__ top, const int *__restrict__ pts,
                                                           const int *__restrict__ near, const long long *__restrict__ frame,
                                                           int G, int step_mm, int min_pts, int *__restrict__ elev,
                                                           int *__restrict__ owner, int *__restrict__ g_out,
                                                           int *__restrict__ info) {
  __shared__ unsigned short s[MAX_G][STRIP];  // bit 15: blocking; after the upward scan the low bits hold the distance up
  __shared__ int s_cnt[2];
  const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.y, j0 = blockIdx.x * STRIP;
  const bool found = load_frame(frame + (size_t)b * NFR).found != 0;
  const size_t off = (size_t)b * G * G;
  if (tid < 2) s_cnt[tid] = 0;
  __syncthreads();
  int known = 0, solid = 0;
  for (int idx = tid; idx < G * STRIP; idx += STRIP * SEGS) {
    const int i = idx / STRIP, jj = idx % STRIP, j = j0 + jj;
    if (j >= G) continue;
    const size_t a = off + (size_t)i * G + j;
    const int t = top[a], np = pts[a];
    const bool sol = found && near[a] >= min_pts;  // near <= pts: a solid cell has a point
    elev[a] = np > 0 ? (t >> 7) - KEY_BIAS : UOC_ELEV_NONE;
    owner[a] = np > 0 ? (t & (NUM_IDS - 1)) : 0;
    known += np > 0;
    solid += sol;
    bool blk = !sol || i == 0 || j == 0 || i == G - 1 || j == G - 1;
    if (!blk) {  // the four edge neighbours lie inside the grid
      const int d[4] = {-G, G, -1, 1};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int t2 = top[a + d[k]];
        const bool ok = near[a + d[k]] >= min_pts && ((t2 ^ t) & (NUM_IDS - 1)) == 0 && abs((t2 >> 7) - (t >> 7)) <= step_mm;
        blk = blk || !ok;
      }
    }
    s[i][jj] = blk ? 0x8000u : 0u;
  }
  known = wave_sum(known);
  solid = wave_sum(solid);
  if (lane == 0) {
    atomicAdd(&s_cnt[0], known);
    atomicAdd(&s_cnt[1], solid);
  }
  __syncthreads();
  if (tid < 2 && s_cnt[tid]) atomicAdd(&info[(size_t)b * 4 + 2 + tid], s_cnt[tid]);
  if (blockIdx.x == 0 && tid == 2) info[(size_t)b * 4] = found ? 1 : 0;
  column_scan(s, G, j0, g_out + off);
}

// ---- 4. the row pass, the per-id table and the queries -----------------------------------------------------------------
struct Acc {
  int *cells, *level, *emax;       // [B][128] each; emax holds elev + KEY_BIAS, 0: none
  unsigned long long *key, *sum;   // [B][128] each; sum is an int64 in two's complement
  unsigned long long *qkey;        // [B][MAX_Q]
};

__global__ __launch_bounds__(ROW_THREADS) void row_kernel(const int *__restrict__ elev, const int *__restrict__ owner,
                                                          const int *__restrict__ near, int G, int min_pts, Queries qs, int Q,
                                                          int *__restrict__ dist2, Acc acc) {
  __shared__ __attribute__((aligned(16))) int s_g2[MAX_G];
  __shared__ unsigned long long s_qkey[MAX_Q];
  __shared__ int s_cells[NUM_IDS], s_level[NUM_IDS], s_emax[NUM_IDS], s_sum[NUM_IDS];  // a row's sum: at most 512 * 32767
  __shared__ unsigned long long s_key[NUM_IDS];
  const int tid = threadIdx.x, lane = tid & 63, i = blockIdx.x, b = blockIdx.y;
  const size_t off = ((size_t)b * G + i) * G;
  row_fill_g2(s_g2, dist2 + off, G);
  if (tid < MAX_Q) s_qkey[tid] = 0ull;
  if (tid < NUM_IDS) {
    s_cells[tid] = s_level[tid] = s_emax[tid] = s_sum[tid] = 0;
    s_key[tid] = 0ull;
  }
  __syncthreads();
  unsigned long long qkey[MAX_Q];
#pragma unroll
  for (int q = 0; q < MAX_Q; ++q) qkey[q] = 0ull;
  for (int jb = 0; jb < G; jb += ROW_THREADS) {  // uniform: every lane takes part in the ballots and shuffles below
    const int j = jb + tid;
    const bool valid = j < G;
    int best = 0, code = -1, el = 0;
    if (valid) {
      best = row_min_dist2(s_g2, j, G);
      dist2[off + j] = best;
      if (near[off + j] >= min_pts) {  // solid
        code = owner[off + j];
        el = elev[off + j];
      }
    }
    const bool lvl = code >= 0 && best > 0;  // not blocking: level
    const unsigned long long wide = lvl ? widest_key(best, i * G + j) : 0ull;
    for_each_wave_key(code, [&](int c, unsigned long long m, int first) {  // per distinct owner of the wave
      const bool hit = code == c;
      const unsigned long long ml = __ballot(hit && lvl);
      const int em = wave_max(hit ? el + KEY_BIAS : 0);
      unsigned long long k64 = 0ull;
      int sm = 0;
      if (ml) {  // uniform
        k64 = wave_max64(hit ? wide : 0ull);
        sm = wave_sum(hit && lvl ? el : 0);
      }
      if (lane == first) {
        atomicAdd(&s_cells[c], __popcll(m));
        atomicMax(&s_emax[c], em);
        if (ml) {
          atomicAdd(&s_level[c], __popcll(ml));
          atomicMax(&s_key[c], k64);
          atomicAdd(&s_sum[c], sm);
        }
      }
    });
    if (Q > 0 && lvl) {
#pragma unroll
      for (int q = 0; q < MAX_Q; ++q) {
        if (q < Q) {  // uniform
          const int id = qs.v[q][1];
          const bool cand = el >= qs.v[q][2] && el <= qs.v[q][3] && (id < 0 ? code >= 1 : code == id);
          qkey[q] = max(qkey[q], cand ? wide : 0ull);
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < MAX_Q; ++q) {
    if (q < Q) {  // uniform
      const unsigned long long k64 = wave_max64(qkey[q]);
      if (lane == 0 && k64) atomicMax(&s_qkey[q], k64);
    }
  }
  __syncthreads();
  if (tid < Q && s_qkey[tid]) atomicMax(&acc.qkey[(size_t)b * MAX_Q + tid], s_qkey[tid]);
  if (tid < NUM_IDS && s_cells[tid]) {
    const size_t a = (size_t)b * NUM_IDS + tid;
    atomicAdd(&acc.cells[a], s_cells[tid]);
    atomicMax(&acc.emax[a], s_emax[tid]);
    if (s_level[tid]) {
      atomicAdd(&acc.level[a], s_level[tid]);
      atomicMax(&acc.key[a], s_key[tid]);
      atomicAdd(&acc.sum[a], (unsigned long long)(long long)s_sum[tid]);
    }
  }
}

// ---- 5. the rows of tops and the answers -------------------------------------------------------------------------------
__global__ __launch_bounds__(NUM_IDS) void answer_kernel(Acc acc, const int *__restrict__ elev, int G, Queries qs, int Q,
                                                    int *__restrict__ tops, int *__restrict__ answers) {
  const int a = threadIdx.x, b = blockIdx.x;
  const size_t r = (size_t)b * NUM_IDS + a;
  const int cells = acc.cells[r], level = acc.level[r];
  int row[8] = {cells, level, -1, -1, 0, 0, cells ? acc.emax[r] - KEY_BIAS : 0, 0};
  if (level) {
    const unsigned long long k64 = acc.key[r];
    const int idx = key_cell(k64);
    row[2] = idx / G;
    row[3] = idx % G;
    row[4] = key_dist2(k64);
    row[5] = elev[(size_t)b * G * G + idx];
    row[7] = (int)floor_div((long long)acc.sum[r], level);
  }
  int *T = tops + r * 8;
#pragma unroll
  for (int k = 0; k < 8; ++k) T[k] = row[k];
  if (a < Q) {
    const unsigned long long k64 = acc.qkey[(size_t)b * MAX_Q + a];
    int4 ans = make_int4(-1, -1, 0, 0);
    if (k64) {
      const int idx = key_cell(k64);
      ans.x = idx / G;
      ans.y = idx % G;
      ans.z = key_dist2(k64);
      ans.w = ans.z >= qs.v[a][0];
    }
    int *A = answers + ((size_t)b * Q + a) * 4;
    A[0] = ans.x;
    A[1] = ans.y;
    A[2] = ans.z;
    A[3] = ans.w;
  }
}

bool shape_ok(int B, int H, int W, int G) { return image_ok(B, H, W) && grid_ok(G); }

struct Ws {
  int *top;  // [B][G][G]
  Acc acc;
  size_t total;
};
Ws carve(void *base, int B, int G) {
  Ws w;
  Carver cv(base);
  w.top = cv.take<int>((size_t)B * G * G);
  w.acc.cells = cv.take<int>((size_t)B * NUM_IDS);
  w.acc.level = cv.take<int>((size_t)B * NUM_IDS);
  w.acc.emax = cv.take<int>((size_t)B * NUM_IDS);
  w.acc.key = cv.take<unsigned long long>((size_t)B * NUM_IDS);
  w.acc.sum = cv.take<unsigned long long>((size_t)B * NUM_IDS);
  w.acc.qkey = cv.take<unsigned long long>((size_t)B * MAX_Q);
  w.total = cv.total();
  return w;
}

template <int PASS>
void launch_points(bool vec, dim3 grid, hipStream_t st, const int32_t *labels, const float *xyz, const long long *frame,
                   long long n, int G, int cell_div, int t_low, int step_mm, int *top, int *pts, int *near, int *info) {
  if (vec)
    hipLaunchKernelGGL((point_kernel<true, PASS>), grid, dim3(256), 0, st, labels, xyz, frame, n, G, cell_div, t_low, step_mm, top,
                       pts, near, info);
  else
    hipLaunchKernelGGL((point_kernel<false, PASS>), grid, dim3(256), 0, st, labels, xyz, frame, n, G, cell_div, t_low, step_mm, top,
                       pts, near, info);
}

}  // namespace
}  // namespace uoc

using namespace uoc;

extern "C" {

size_t uoc_elevation_workspace_bytes(int B, int H, int W, int G) {
  if (!shape_ok(B, H, W, G)) return 0;
  return carve(nullptr, B, G).total;
}

int uoc_elevation(const int32_t *d_labels, const float *d_xyz, const int64_t *d_frame, int B, int H, int W, int G, int cell_mm,
                  int tau_mm, int step_mm, int min_pts, const int32_t *h_queries, int Q, int32_t *d_elev, int32_t *d_owner,
                  int32_t *d_pts, int32_t *d_near, int32_t *d_dist2, int32_t *d_tops, int32_t *d_info, int32_t *d_answers,
                  void *d_ws, size_t ws_bytes, void *stream) {
  UOC_REQUIRE(d_labels && d_xyz && d_frame && d_elev && d_owner && d_pts && d_near && d_dist2 && d_tops && d_info && d_ws,
              "uoc_elevation: null labels / xyz / frame / elev / owner / pts / near / dist2 / tops / info / workspace");
  UOC_REQUIRE(image_ok(B, H, W),
              "uoc_elevation: bad shape B=%d H=%d W=%d (B in 1..65535, H*W below 2^31)", B, H, W);
  UOC_REQUIRE(grid_ok(G), "uoc_elevation: grid = %d is not a multiple of 8 in [8, %d]", G, MAX_G);
  UOC_REQUIRE(cell_mm >= 1 && cell_mm <= 1000, "uoc_elevation: cell_mm = %d outside [1, 1000]", cell_mm);
  UOC_REQUIRE(tau_mm >= 1 && tau_mm <= 1000, "uoc_elevation: tau_mm = %d outside [1, 1000]", tau_mm);
  UOC_REQUIRE(step_mm >= 1 && step_mm <= 1000, "uoc_elevation: step_mm = %d outside [1, 1000]", step_mm);
  UOC_REQUIRE(min_pts >= 1 && min_pts <= 65535, "uoc_elevation: min_pts = %d outside [1, 65535]", min_pts);
  UOC_REQUIRE(Q >= 0 && Q <= MAX_Q, "uoc_elevation: %d queries outside [0, %d]", Q, MAX_Q);
  UOC_REQUIRE(Q == 0 || (h_queries && d_answers), "uoc_elevation: null queries / answers with Q = %d", Q);
  Queries qs;
  for (int q = 0; q < MAX_Q; ++q)
    for (int k = 0; k < 4; ++k) qs.v[q][k] = q < Q ? h_queries[q * 4 + k] : 0;
  for (int q = 0; q < Q; ++q) {
    UOC_REQUIRE(qs.v[q][0] >= 0 && qs.v[q][0] <= (1 << 30), "uoc_elevation: query %d: need2 = %d outside [0, 2^30]", q, qs.v[q][0]);
    UOC_REQUIRE(qs.v[q][1] >= -1 && qs.v[q][1] < NUM_IDS, "uoc_elevation: query %d: id = %d outside [-1, 127]", q, qs.v[q][1]);
    UOC_REQUIRE(qs.v[q][2] >= -32768 && qs.v[q][2] <= 32767 && qs.v[q][3] >= -32768 && qs.v[q][3] <= 32767,
                "uoc_elevation: query %d: band (%d, %d) outside [-32768, 32767]", q, qs.v[q][2], qs.v[q][3]);
  }
  const Ws w = carve(d_ws, B, G);
  UOC_REQUIRE(ws_bytes >= w.total, "uoc_elevation: workspace %zu < %zu bytes", ws_bytes, w.total);
  UOC_REQUIRE(aligned16(d_ws), "uoc_elevation: workspace not 16-byte aligned");
  const long long n = (long long)H * W;
  const int nch = (int)((n + PIX_CHUNK - 1) / PIX_CHUNK);
  const size_t cells = (size_t)B * G * G;
  const bool vec = n % 4 == 0 && (((uintptr_t)d_labels | (uintptr_t)d_xyz) & 15) == 0;
  const long long *frame = (const long long *)d_frame;
  hipStream_t st = (hipStream_t)stream;
  {
    ProfScope prof(KC_ELEV_RASTER, st, 0.0, (double)B * n * 32.0 + (double)cells * 24.0);
    UOC_HIP_CHECK(hipMemsetAsync(d_ws, 0, w.total, st));
    UOC_HIP_CHECK(hipMemsetAsync(d_pts, 0, cells * sizeof(int32_t), st));
    UOC_HIP_CHECK(hipMemsetAsync(d_near, 0, cells * sizeof(int32_t), st));
    UOC_HIP_CHECK(hipMemsetAsync(d_info, 0, (size_t)B * 4 * sizeof(int32_t), st));
    launch_points<1>(vec, dim3(nch, B), st, d_labels, d_xyz, frame, n, G, cell_mm * SCALE, -tau_mm * SCALE, step_mm, w.top, d_pts,
                     d_near, d_info);
    launch_points<2>(vec, dim3(nch, B), st, d_labels, d_xyz, frame, n, G, cell_mm * SCALE, -tau_mm * SCALE, step_mm, w.top, d_pts,
                     d_near, d_info);
  }
  {
    ProfScope prof(KC_ELEV_TRANSFORM, st, (double)cells * G * 3.0, (double)cells * 52.0);
    hipLaunchKernelGGL(cell_kernel, dim3((G + STRIP - 1) / STRIP, B), dim3(STRIP * SEGS), 0, st, w.top, d_pts, d_near, frame, G,
                       step_mm, min_pts, d_elev, d_owner, d_dist2, d_info);
    hipLaunchKernelGGL(row_kernel, dim3(G, B), dim3(ROW_THREADS), 0, st, d_elev, d_owner, d_near, G, min_pts, qs, Q, d_dist2, w.acc);
    hipLaunchKernelGGL(answer_kernel, dim3(B), dim3(NUM_IDS), 0, st, w.acc, d_elev, G, qs, Q, d_tops, d_answers);
  }
  UOC_LAUNCH_CHECK();
  return UOC_OK;
}

}  // extern "C"
