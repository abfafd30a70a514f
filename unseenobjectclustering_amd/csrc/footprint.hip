// Footprint fitting: oriented put-down poses on the table grid (include/uoc_hip.h, uoc_footprint).
// From the state / owner / dist2 grids and the frame records of uoc_placement, a host table of A directions and up to 8
// rectangle records: per cell and rectangle the set of directions in which the rectangle, centred on the cell, lies
// wholly on free cells (fits, one bit per direction), the cells per direction (count) and the best pose (best).
// Integers only.
//
// Two memsets (the accumulators in the workspace, d_count) and four launches:
//   span_kernel    one thread per (rectangle f, direction k, mask row di): it scans dj over the window and writes the
//                  row's span (dj_lo, dj_hi) as two signed bytes, (1, 0) for an empty row.  The mask is an intersection of
//                  half planes, so a row of it is one span.  Independent of the frame: once per call.
//   run_kernel     (grid.h) grid (rows, tables, frames), 4 waves.  A table belongs to one value of `ignore`; rectangles with the
//                  same value share it.  The row's FREE bits by ballot into LDS (8 words of 64 at G = 512), then per cell
//                  the length of the run of FREE cells that ends there, by counting leading ones: 16-bit words.  A frame
//                  without a plane gets a table of zeros, which makes everything downstream of it zero.
//   fit_kernel     grid (chunks of 256 cells, rectangles, frames), 16 waves: 256 cells x 4 groups of directions (k = g,
//                  g + 4, ...), so that a frame alone still fills the machine.  The rectangle's span table in LDS (2 bytes
//                  per row: 8.4 KB at the limits).  A thread owns a cell and a group; a cell with run == 0 is not FREE
//                  and has no pose.  Per direction and non-empty row one 16-bit read: the span [j+lo, j+hi] of row i+di is
//                  free iff it lies in the grid and run[i+di][j+hi] >= hi-lo+1.  The run rows come from L2 (a table is
//                  128 KB at G = 256); neighbouring lanes read neighbouring words.  Eight rows are read at a time, their
//                  reads independent of one another, and the wave leaves a direction when none of its lanes is left; a
//                  loop that leaves at the first failing row issues one dependent L2 read per row, and that chain bounds
//                  a single frame (DESIGN.md section 18 has the measurement).  The groups' words meet by an LDS atomicOr.  count: ballot and popcount per direction per wave, an LDS
//                  table, integer atomicAdd.  The key: maximum per wave by shuffles, per block by an LDS atomicMax, per
//                  (frame, rectangle) by a 64-bit atomicMax.
//   answer_kernel  one thread per (frame, rectangle): the key, the counts and the cells into best.
//
// Determinism: integer adds and maxima commute and the key is a strict total order over (cell, k), so no result depends
// on the order in which lanes, waves or blocks arrive.  Nothing of frame b depends on the other frames of the batch.
#include "grid.h"
#include "prof.h"

namespace uoc {
namespace {

constexpr int UNIT = 256;     // a half extent counts 1/256 cell; S / UNIT = 64
constexpr int MAX_A = 32, MAX_F = UOC_FOOT_MAX_RECTS, MAX_HALF = UOC_FOOT_MAX_HALF;
constexpr int MAX_R = 64;                  // (256 * 64)^2 = MAX_HALF^2
constexpr int MAX_ROWS = 2 * MAX_R + 3;    // the window is |di| <= R + 1: 131 rows
constexpr int THREADS = 256;
constexpr int CELLS = 256, KGROUPS = 4, FIT_THREADS = CELLS * KGROUPS, BATCH = 8;  // fit_kernel: cells per block, groups of directions
constexpr int DIST_CAP = 65536;

static_assert((long long)(MAX_R + 1) * SCALE * 2 < (1 << 22), "a projection stays below 2^22");
static_assert(MAX_R + 1 <= 127, "a span is two signed bytes");

struct Dirs {
  int c[MAX_A][2];  // (Cx, Cy)
};
struct Rects {
  int v[MAX_F][8];  // HL, HW, ignore, mode, ai, aj, 0, 0
};
struct Plan {
  int R[MAX_F];       // R_f
  int table[MAX_F];   // the run table of rectangle f
  RunIgnore<MAX_F> ignore;  // the `ignore` of table t
};

// ---- 1. the spans of the masks ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void span_kernel(Dirs d, Rects r, Plan p, int A, int F, signed char *__restrict__ spans) {
  const int t = blockIdx.x * THREADS + threadIdx.x;
  if (t >= F * A * MAX_ROWS) return;
  const int f = t / (A * MAX_ROWS), k = (t / MAX_ROWS) % A, di = t % MAX_ROWS - (MAX_R + 1);
  const int win = p.R[f] + 1, cx = d.c[k][0], cy = d.c[k][1];
  const int lim_l = (SCALE / UNIT) * r.v[f][0], lim_w = (SCALE / UNIT) * r.v[f][1];
  int lo = 1, hi = 0;  // empty
  if (abs(di) <= win) {
    bool any = false;
    for (int dj = -win; dj <= win; ++dj) {
      if (abs(di * cx + dj * cy) <= lim_l && abs(-di * cy + dj * cx) <= lim_w) {
        if (!any) lo = dj;
        hi = dj;
        any = true;
      }
    }
  }
  spans[2 * t] = (signed char)lo;
  spans[2 * t + 1] = (signed char)hi;
}

// ---- 3. the fit -------------------------------------------------------------------------------------------------------
struct Acc {
  unsigned long long *key;  // [B][F]
  int *cells;               // [B][F]
};

__global__ __launch_bounds__(FIT_THREADS) void fit_kernel(const unsigned short *__restrict__ runs, const int *__restrict__ dist2,
                                                          const signed char *__restrict__ spans, int G, int A, int F, int NT,
                                                          Rects r, Plan p, int *__restrict__ fits, int *__restrict__ count, Acc acc) {
  __shared__ short s_span[MAX_A * MAX_ROWS];  // (hi << 8) | (lo & 255) of row (k, di + R + 1)
  __shared__ unsigned s_word[CELLS];
  __shared__ int s_count[MAX_A];
  __shared__ int s_cells;
  __shared__ unsigned long long s_key;
  const int tid = threadIdx.x, lane = tid & 63, c = tid & (CELLS - 1), kg = tid / CELLS;  // a wave has one kg
  const int f = blockIdx.y, b = blockIdx.z;
  const int win = p.R[f] + 1, rows = 2 * win + 1;
  const int cells = G * G;
  const int idx = blockIdx.x * CELLS + c;  // G*G is a multiple of 64: a wave is inside or outside as a whole
  const unsigned short *run = runs + ((size_t)b * NT + p.table[f]) * cells;
  const int own = idx < cells ? run[idx] : 0;
  if (__syncthreads_or(own) == 0) {  // no FREE cell in the chunk: nothing to count
    if (kg == 0 && idx < cells) fits[((size_t)b * F + f) * cells + idx] = 0;
    return;
  }
  for (int e = tid; e < A * rows; e += FIT_THREADS) {
    const int k = e / rows, row = e - k * rows;
    const signed char *sp = spans + 2 * ((size_t)(f * A + k) * MAX_ROWS + (row - win + MAX_R + 1));
    s_span[e] = (short)(((int)sp[1] << 8) | ((int)sp[0] & 255));
  }
  if (tid < CELLS) s_word[tid] = 0u;
  if (tid < MAX_A) s_count[tid] = 0;
  if (tid == 0) {
    s_cells = 0;
    s_key = 0ull;
  }
  __syncthreads();
  const int i = idx / G, j = idx - i * G;
  unsigned word = 0u;
  for (int k = kg; k < A; k += KGROUPS) {  // uniform per wave
    const short *sp = s_span + k * rows;   // sp[di + win]
    bool ok = own != 0;
    for (int r0 = 0; r0 < rows && __any(ok); r0 += BATCH) {
      // BATCH rows at a time, their reads independent of one another: a row's word comes from L2, and one dependent
      // read per row would be a chain of L2 latencies.  A read outside the grid goes to the cell's own word instead.  A
      // lane whose cell is not FREE (own == 0) in a wave that is still alive issues the eight clamped reads all the
      // same, to its own word, until __any(ok) drops: the wave's read costs the same with or without that lane.
      int v[BATCH], need[BATCH];
#pragma unroll
      for (int u = 0; u < BATCH; ++u) {
        const int row = r0 + u;
        const int s = row < rows ? sp[row] : 1;  // 1: lo = 1, hi = 0, an empty row
        const int lo = (signed char)(s & 255), hi = s >> 8;
        const int ii = i + row - win, j1 = j + hi;
        const bool inside = (unsigned)ii < (unsigned)G && j + lo >= 0 && j1 < G && lo <= hi && own != 0;
        need[u] = hi - lo + 1;  // 0 for an empty row
        v[u] = inside ? ii * G + j1 : -1;
      }
#pragma unroll
      for (int u = 0; u < BATCH; ++u) {
        const int got = run[v[u] >= 0 ? v[u] : min(idx, cells - 1)];
        v[u] = v[u] >= 0 ? got : 0;
      }
#pragma unroll
      for (int u = 0; u < BATCH; ++u) ok = ok && v[u] >= need[u];
    }
    word |= ok ? (1u << k) : 0u;
  }
  if (word) atomicOr(&s_word[c], word);
  __syncthreads();
  unsigned long long key = 0ull;
  if (kg == 0) {  // whole waves
    word = s_word[c];
    if (idx < cells) fits[((size_t)b * F + f) * cells + idx] = (int)word;
    if (word) {
      const int k = __ffs((int)word) - 1;  // the lowest direction carries the cell's largest key
      const unsigned long long low = (cell_key(idx) << 5) | (unsigned long long)(31 - k);
      if (r.v[f][3] == UOC_FOOT_NEAREST) {
        const int ei = i - r.v[f][4], ej = j - r.v[f][5];
        key = ((unsigned long long)((1 << 27) - 1 - (ei * ei + ej * ej)) << 23) | low;
      } else {
        const int dd = min(max(dist2[(size_t)b * cells + idx], 0), DIST_CAP);
        key = ((unsigned long long)(dd + 1) << 23) | low;
      }
    }
    const unsigned long long any = __ballot(word != 0u);
    if (any) {  // uniform per wave
      for (int k = 0; k < A; ++k) {
        const int n = __popcll(__ballot((word >> k) & 1u));
        if (lane == 0 && n) atomicAdd(&s_count[k], n);
      }
      key = wave_max64(key);
      if (lane == 0) {
        atomicAdd(&s_cells, (int)__popcll(any));
        atomicMax(&s_key, key);
      }
    }
  }
  const size_t bf = (size_t)b * F + f;
  __syncthreads();
  if (tid < A && s_count[tid]) atomicAdd(&count[bf * 32 + tid], s_count[tid]);
  if (tid == 32 && s_cells) {
    atomicAdd(&acc.cells[bf], s_cells);
    atomicMax(&acc.key[bf], s_key);
  }
}

// ---- 4. the best records ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void answer_kernel(Acc acc, const int *__restrict__ count, const int *__restrict__ dist2, int G,
                                                    int A, int F, int n, Rects r, int *__restrict__ best) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= n) return;
  const int f = t % F, b = t / F;
  const unsigned long long key = acc.key[t];
  int row[8] = {0, -1, -1, -1, 0, 0, 0, 0};
  if (key) {
    const int idx = key_cell(key >> 5);
    const int i = idx / G, j = idx - i * G, ei = i - r.v[f][4], ej = j - r.v[f][5];
    int poses = 0;
    for (int k = 0; k < A; ++k) poses += count[(size_t)t * 32 + k];
    row[0] = 1;
    row[1] = i;
    row[2] = j;
    row[3] = 31 - (int)(key & 31ull);
    row[4] = min(max(dist2[(size_t)b * G * G + idx], 0), DIST_CAP);
    row[5] = ei * ei + ej * ej;
    row[6] = poses;
    row[7] = acc.cells[t];
  }
  int *o = best + (size_t)t * 8;
#pragma unroll
  for (int k = 0; k < 8; ++k) o[k] = row[k];
}

bool shape_ok(int B, int G, int A, int F) {
  return batch_ok(B) && grid_ok(G) && A >= 1 && A <= MAX_A && F >= 1 && F <= MAX_F;
}

struct Ws {
  signed char *spans;    // [F][A][131][2]
  unsigned short *runs;  // room for [B][F][G][G]; a call packs its NT <= F tables per frame: [B][NT][G][G]
  Acc acc;
  size_t acc_at, acc_bytes, total;
};
Ws carve(void *base, int B, int G, int A, int F) {
  Ws w;
  Carver cv(base);
  w.spans = cv.take<signed char>((size_t)F * A * MAX_ROWS * 2);
  w.runs = cv.take<unsigned short>((size_t)B * F * G * G);
  w.acc_at = cv.total();
  w.acc.key = cv.take<unsigned long long>((size_t)B * F);
  w.acc.cells = cv.take<int>((size_t)B * F);
  w.acc_bytes = cv.total() - w.acc_at;
  w.total = cv.total();
  return w;
}

}  // namespace
}  // namespace uoc

using namespace uoc;

extern "C" {

size_t uoc_footprint_workspace_bytes(int B, int G, int A, int F) {
  if (!shape_ok(B, G, A, F)) return 0;
  return carve(nullptr, B, G, A, F).total;
}

int uoc_footprint(const int32_t *d_state, const int32_t *d_owner, const int32_t *d_dist2, const int64_t *d_frame, int B, int G,
                  const int32_t *h_dirs, int A, const int32_t *h_rects, int F, int unknown_blocks, int32_t *d_fits,
                  int32_t *d_count, int32_t *d_best, void *d_ws, size_t ws_bytes, void *stream) {
  UOC_REQUIRE(d_state && d_owner && d_dist2 && h_dirs && h_rects && d_fits && d_count && d_best && d_ws,
              "uoc_footprint: null state / owner / dist2 / dirs / rects / fits / count / best / workspace");
  UOC_REQUIRE(batch_ok(B), "uoc_footprint: bad shape B=%d (B in 1..65535)", B);
  UOC_REQUIRE(grid_ok(G), "uoc_footprint: grid = %d is not a multiple of 8 in [8, %d]", G, MAX_G);
  UOC_REQUIRE(A >= 1 && A <= MAX_A, "uoc_footprint: %d directions outside [1, %d]", A, MAX_A);
  UOC_REQUIRE(F >= 1 && F <= MAX_F, "uoc_footprint: %d rectangles outside [1, %d]", F, MAX_F);
  UOC_REQUIRE(unknown_blocks == 0 || unknown_blocks == 1, "uoc_footprint: unknown_blocks = %d is neither 0 nor 1", unknown_blocks);
  Dirs d;
  for (int k = 0; k < MAX_A; ++k)
    for (int c = 0; c < 2; ++c) d.c[k][c] = k < A ? h_dirs[k * 2 + c] : 0;
  for (int k = 0; k < A; ++k)
    UOC_REQUIRE(d.c[k][0] >= -SCALE && d.c[k][0] <= SCALE && d.c[k][1] >= -SCALE && d.c[k][1] <= SCALE,
                "uoc_footprint: direction %d = (%d, %d) has a component outside [-%d, %d]", k, d.c[k][0], d.c[k][1], SCALE, SCALE);
  Rects r;
  Plan p;
  int NT = 0;
  for (int f = 0; f < MAX_F; ++f) {
    for (int k = 0; k < 8; ++k) r.v[f][k] = f < F ? h_rects[f * 8 + k] : 0;
    p.R[f] = p.table[f] = p.ignore.v[f] = 0;
  }
  for (int f = 0; f < F; ++f) {
    const int *v = r.v[f];
    UOC_REQUIRE(v[0] >= 0 && v[0] <= MAX_HALF && v[1] >= 0 && v[1] <= MAX_HALF,
                "uoc_footprint: rectangle %d: half extents HL = %d, HW = %d outside [0, %d]", f, v[0], v[1], MAX_HALF);
    const long long q = (long long)v[0] * v[0] + (long long)v[1] * v[1];
    UOC_REQUIRE(q <= (long long)MAX_HALF * MAX_HALF, "uoc_footprint: rectangle %d: HL^2 + HW^2 = %lld above %d^2", f, q, MAX_HALF);
    UOC_REQUIRE(v[2] >= 0 && v[2] < NUM_IDS, "uoc_footprint: rectangle %d: ignore = %d outside [0, 127]", f, v[2]);
    UOC_REQUIRE(v[3] == UOC_FOOT_ROOMIEST || v[3] == UOC_FOOT_NEAREST, "uoc_footprint: rectangle %d: mode = %d is neither 0 nor 1", f, v[3]);
    UOC_REQUIRE(v[4] >= -MAX_ANCHOR && v[4] < MAX_ANCHOR && v[5] >= -MAX_ANCHOR && v[5] < MAX_ANCHOR,
                "uoc_footprint: rectangle %d: anchor (ai, aj) = (%d, %d) outside [-%d, %d]", f, v[4], v[5], MAX_ANCHOR, MAX_ANCHOR - 1);
    UOC_REQUIRE(v[6] == 0 && v[7] == 0, "uoc_footprint: rectangle %d: reserved words (%d, %d) are not zero", f, v[6], v[7]);
    int R = 0;
    while ((long long)(UNIT * R) * (UNIT * R) < q) ++R;  // at most 64
    p.R[f] = R;
    int t = 0;
    while (t < NT && p.ignore.v[t] != v[2]) ++t;
    if (t == NT) p.ignore.v[NT++] = v[2];
    p.table[f] = t;
  }
  const Ws w = carve(d_ws, B, G, A, F);
  UOC_REQUIRE(ws_bytes >= w.total, "uoc_footprint: workspace %zu < %zu bytes", ws_bytes, w.total);
  UOC_REQUIRE(aligned16(d_ws), "uoc_footprint: workspace not 16-byte aligned");
  const int cells = G * G, nspan = F * A * MAX_ROWS;
  hipStream_t st = (hipStream_t)stream;
  {
    ProfScope prof(KC_FOOT_TABLES, st, 0.0, (double)B * cells * (8.0 + 2.0 * NT));
    UOC_HIP_CHECK(hipMemsetAsync((char *)d_ws + w.acc_at, 0, w.acc_bytes, st));
    UOC_HIP_CHECK(hipMemsetAsync(d_count, 0, (size_t)B * F * 32 * sizeof(int32_t), st));
    hipLaunchKernelGGL(span_kernel, dim3((nspan + THREADS - 1) / THREADS), dim3(THREADS), 0, st, d, r, p, A, F, w.spans);
    hipLaunchKernelGGL(run_kernel<MAX_F>, dim3(G, NT, B), dim3(RUN_THREADS), 0, st, d_state, d_owner, (const long long *)d_frame, G,
                       NT, p.ignore, unknown_blocks, w.runs);
  }
  {
    ProfScope prof(KC_FOOT_FIT, st, 0.0, (double)B * F * cells * 10.0);
    hipLaunchKernelGGL(fit_kernel, dim3((cells + CELLS - 1) / CELLS, F, B), dim3(FIT_THREADS), 0, st, w.runs, d_dist2, w.spans, G, A, F,
                       NT, r, p, d_fits, d_count, w.acc);
    hipLaunchKernelGGL(answer_kernel, dim3((B * F + 63) / 64), dim3(64), 0, st, w.acc, d_count, d_dist2, G, A, F, B * F, r, d_best);
  }
  UOC_LAUNCH_CHECK();
  return UOC_OK;
}

}  // extern "C"
