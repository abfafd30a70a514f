// Object motion: planar registration on the table grid (include/uoc_hip.h, uoc_motion).
// From the state / owner grids of two placements of the same frames, rasterised in one plane frame, a host table of A
// rotations over a full turn, a radius R and up to 16 pairs (id_a, id_b): per pair the rotation k and the shift s that
// minimise the number of cells the turned and shifted "before" mask and the "after" mask do not share, counted both
// ways (rot, best).  Integers only.
//
// One memset (the heads and the keys in the workspace) and three launches:
//   gather_kernel  grid (chunks of 1024 cells, pairs, frames), 4 waves.  A thread reads its four cells of both grids, all
//                  loads first; the members of each mask go to the pair's cell list by a ballot and one atomicAdd per
//                  wave and turn, the counts past UOC_MOTION_MAX_CELLS are kept and their cells dropped (status 3).  The
//                  sums for the pivots and the cells in both masks: per lane over its turns, per wave by shuffles, one
//                  atomicAdd per wave.  A frame without a common frame record adds nothing: its counts stay 0.
//   search_kernel  grid (rotations x NS, pairs, frames), 16 waves, everything in dynamic LDS: the two masks as bit planes
//                  (2 x G*G/8 bytes, built from the lists), A's cells turned by this block's k and moved to q as packed
//                  16-bit pairs, B's cells as the two unrounded inverse products (the shift's products are subtracted
//                  before the rounding, which is exact: rd rounds a sum the shift enters linearly).  Waves take shifts
//                  round-robin, lanes stride the two lists and count misses; a target outside the grid is a miss before
//                  any index is formed.  A wave keeps its least key in a register and ends with one 64-bit LDS atomicMin,
//                  the block with one 64-bit atomicMax of the key's complement on the rotation's word in the workspace.
//                  With fewer than 1024 (rotation, pair, frame) triples the host shares the shifts of a rotation among
//                  NS <= 16 blocks: one pair of one frame alone would leave seven compute units in eight idle.
//   answer_kernel  one wave per (frame, pair), a lane per rotation: the rot rows from the keys, the status, the least key
//                  over k and `second` by shuffles, best by lane 0.
//
// Determinism: integer adds and minima commute, the key is a strict total order over (k, s) and no result depends on the
// order of a cell list, so nothing depends on the order in which lanes, waves or blocks arrive.  Nothing of frame b
// depends on the other frames of the batch, nothing of pair p on the other pairs.
#include "grid.h"

#include <algorithm>

namespace uoc {
namespace {

constexpr int MAX_A = UOC_MOTION_MAX_ROT, MAX_R = UOC_MOTION_MAX_RADIUS, MAX_P = UOC_MOTION_MAX_PAIRS;
constexpr int MAX_CELLS = UOC_MOTION_MAX_CELLS;
constexpr int GATHER_THREADS = 256, GATHER_TURNS = 4, GATHER_CHUNK = GATHER_THREADS * GATHER_TURNS;
constexpr int SEARCH_THREADS = 1024, SEARCH_WAVES = SEARCH_THREADS / 64;
constexpr int HEAD = 8;  // words of a pair's head: n_a, n_b, sum i_a, sum j_a, sum i_b, sum j_b, |A n B|, 0
constexpr int H_NA = 0, H_NB = 1, H_IA = 2, H_JA = 3, H_IB = 4, H_JB = 5, H_BOTH = 6;

static_assert(SCALE == UOC_MOTION_SCALE, "the rotation table shares S with the frame");
static_assert((long long)(MAX_G + MAX_R) * SCALE < (1 << 24), "a product stays below 2^24");
static_assert((long long)MAX_G * MAX_G * MAX_G < (1ll << 31), "a coordinate sum fits an int");
static_assert(2 * MAX_G + MAX_R < 32767, "a turned cell moved to the other pivot fits 16 bits");
static_assert((-3 >> 1) == -2, "rd relies on an arithmetic right shift");
static_assert((2 * MAX_R + 1) * (2 * MAX_R + 1) <= 2048 && MAX_A <= 64 && 2 * MAX_R * MAX_R < 1024, "the key's fields");

struct Table {
  int c[MAX_A][2];  // (Cx, Cy)
};
struct Pairs {
  int v[MAX_P][2];  // (id_a, id_b)
};

// Step S, status 0: with records given, both found words are 1 and the 16 words agree.  Uniform per frame.
__device__ __forceinline__ bool common_frame(const long long *__restrict__ fa, const long long *__restrict__ fb, int b) {
  if (fa == nullptr) return true;
  const long long *x = fa + (size_t)b * NFR, *y = fb + (size_t)b * NFR;
  bool ok = x[FR_FOUND] == 1 && y[FR_FOUND] == 1;
  for (int k = 0; k < NFR; ++k) ok = ok && x[k] == y[k];
  return ok;
}

__device__ __forceinline__ int rd(int x) { return (2 * x + SCALE) >> 15; }  // floor_div(2x + S, 2S)
__device__ __forceinline__ int pivot(int sum, int n) { return (int)floor_div(2ll * sum + n, 2 * n); }

__device__ __forceinline__ unsigned long long motion_key(int cost, int si, int sj, int k, int A, int R) {
  const int s2 = si * si + sj * sj, kk = min(k, A - k), sidx = (si + R) * (2 * R + 1) + (sj + R);
  return ((unsigned long long)cost << 33) | ((unsigned long long)s2 << 23) | ((unsigned long long)kk << 17) |
         ((unsigned long long)k << 11) | (unsigned long long)sidx;
}

// ---- 1. the cell lists, the counts and the sums -----------------------------------------------------------------------
__global__ __launch_bounds__(GATHER_THREADS) void gather_kernel(const int *__restrict__ state_a, const int *__restrict__ owner_a,
                                                                const long long *__restrict__ frame_a, const int *__restrict__ state_b,
                                                                const int *__restrict__ owner_b, const long long *__restrict__ frame_b,
                                                                int G, int P, Pairs pairs, int *__restrict__ heads,
                                                                unsigned *__restrict__ lists) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int p = blockIdx.y, b = blockIdx.z;
  if (!common_frame(frame_a, frame_b, b)) return;
  const int ida = pairs.v[p][0], idb = pairs.v[p][1];
  const int cells = G * G;
  const size_t bp = (size_t)b * P + p;
  int *head = heads + bp * HEAD;
  unsigned *list_a = lists + bp * 2 * MAX_CELLS, *list_b = list_a + MAX_CELLS;
  const int *sa = state_a + (size_t)b * cells, *oa = owner_a + (size_t)b * cells;
  const int *sb = state_b + (size_t)b * cells, *ob = owner_b + (size_t)b * cells;
  int sum_ia = 0, sum_ja = 0, sum_ib = 0, sum_jb = 0, both = 0;
  bool in_a[GATHER_TURNS], in_b[GATHER_TURNS];
#pragma unroll
  for (int t = 0; t < GATHER_TURNS; ++t) {  // the loads of every turn first: independent of one another
    const int idx = blockIdx.x * GATHER_CHUNK + t * GATHER_THREADS + tid;
    const bool inside = idx < cells;
    in_a[t] = inside && sa[idx] == 2 && oa[idx] == ida;
    in_b[t] = inside && sb[idx] == 2 && ob[idx] == idb;
  }
#pragma unroll
  for (int t = 0; t < GATHER_TURNS; ++t) {
    const int idx = blockIdx.x * GATHER_CHUNK + t * GATHER_THREADS + tid;
    const int i = idx / G, j = idx - i * G;
    const unsigned word = ((unsigned)i << 16) | (unsigned)j;
    const unsigned long long ma = __ballot(in_a[t]), mb = __ballot(in_b[t]);
    if (ma) {
      int base = 0;
      if (lane == 0) base = atomicAdd(&head[H_NA], (int)__popcll(ma));
      const int at = __shfl(base, 0) + lane_rank(ma);
      if (in_a[t] && at < MAX_CELLS) list_a[at] = word;
    }
    if (mb) {
      int base = 0;
      if (lane == 0) base = atomicAdd(&head[H_NB], (int)__popcll(mb));
      const int at = __shfl(base, 0) + lane_rank(mb);
      if (in_b[t] && at < MAX_CELLS) list_b[at] = word;
    }
    sum_ia += in_a[t] ? i : 0;
    sum_ja += in_a[t] ? j : 0;
    sum_ib += in_b[t] ? i : 0;
    sum_jb += in_b[t] ? j : 0;
    both += in_a[t] && in_b[t] ? 1 : 0;
  }
  sum_ia = wave_sum(sum_ia);
  sum_ja = wave_sum(sum_ja);
  sum_ib = wave_sum(sum_ib);
  sum_jb = wave_sum(sum_jb);
  both = wave_sum(both);
  if (lane == 0) {
    if (sum_ia) atomicAdd(&head[H_IA], sum_ia);
    if (sum_ja) atomicAdd(&head[H_JA], sum_ja);
    if (sum_ib) atomicAdd(&head[H_IB], sum_ib);
    if (sum_jb) atomicAdd(&head[H_JB], sum_jb);
    if (both) atomicAdd(&head[H_BOTH], both);
  }
}

// ---- 2. the search ----------------------------------------------------------------------------------------------------
// The dynamic LDS of a block: the key, the two bit planes, the turned list of A and the products of B.
__host__ __device__ constexpr size_t search_lds_bytes(int G) {
  return 16 + 2 * (size_t)(G * G / 8) + (size_t)MAX_CELLS * 4 + (size_t)MAX_CELLS * 8;
}

__global__ __launch_bounds__(SEARCH_THREADS) void search_kernel(const int *__restrict__ heads, const unsigned *__restrict__ lists, int G,
                                                                int A, int R, int P, int NS, Table table,
                                                                unsigned long long *__restrict__ keys) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k = blockIdx.x / NS, slice = blockIdx.x - k * NS, p = blockIdx.y, b = blockIdx.z;
  const size_t bp = (size_t)b * P + p;
  const int *head = heads + bp * HEAD;
  const int na = head[H_NA], nb = head[H_NB];
  if (na < 1 || nb < 1 || na > MAX_CELLS || nb > MAX_CELLS) return;  // uniform per block: status 0, 2 or 3, the key stays 0
  const int words = G * G / 32;
  unsigned long long *s_key = reinterpret_cast<unsigned long long *>(smem);
  unsigned *s_a = reinterpret_cast<unsigned *>(smem + 16), *s_b = s_a + words;
  unsigned *s_fwd = s_b + words;                                // (ti << 16) | (tj & 0xFFFF) of q + F_k(c - p)
  int2 *s_inv = reinterpret_cast<int2 *>(s_fwd + MAX_CELLS);    // the inverse products of c' - q
  const unsigned *list_a = lists + bp * 2 * MAX_CELLS, *list_b = list_a + MAX_CELLS;
  const int pi = pivot(head[H_IA], na), pj = pivot(head[H_JA], na), qi = pivot(head[H_IB], nb), qj = pivot(head[H_JB], nb);
  const int cx = table.c[k][0], cy = table.c[k][1];
  for (int e = tid; e < 2 * words; e += SEARCH_THREADS) s_a[e] = 0u;
  if (tid == 0) *s_key = ~0ull;
  __syncthreads();
  for (int e = tid; e < na; e += SEARCH_THREADS) {
    const unsigned w = list_a[e];
    const int i = (int)(w >> 16), j = (int)(w & 0xFFFFu), idx = i * G + j;
    atomicOr(&s_a[idx >> 5], 1u << (idx & 31));
    const int di = i - pi, dj = j - pj;
    const int ti = qi + rd(di * cx - dj * cy), tj = qj + rd(di * cy + dj * cx);
    s_fwd[e] = ((unsigned)ti << 16) | ((unsigned)tj & 0xFFFFu);
  }
  for (int e = tid; e < nb; e += SEARCH_THREADS) {
    const unsigned w = list_b[e];
    const int i = (int)(w >> 16), j = (int)(w & 0xFFFFu), idx = i * G + j;
    atomicOr(&s_b[idx >> 5], 1u << (idx & 31));
    const int ei = i - qi, ej = j - qj;
    s_inv[e] = make_int2(ei * cx + ej * cy, -ei * cy + ej * cx);
  }
  __syncthreads();
  const int side = 2 * R + 1, shifts = side * side;
  unsigned long long best = ~0ull;
  for (int t = slice * SEARCH_WAVES + wave; t < shifts; t += NS * SEARCH_WAVES) {  // uniform per wave
    const int si = t / side - R, sj = t - (t / side) * side - R;
    const int su = si * cx + sj * cy, sv = -si * cy + sj * cx;
    int miss = 0;
    for (int e = lane; e < na; e += 64) {
      const unsigned w = s_fwd[e];
      const int ti = ((int)w >> 16) + si, tj = (int)(short)(w & 0xFFFFu) + sj;
      bool hit = false;
      if ((unsigned)ti < (unsigned)G && (unsigned)tj < (unsigned)G) {  // inside the grid, only then an index
        const int idx = ti * G + tj;
        hit = (s_b[idx >> 5] >> (idx & 31)) & 1u;
      }
      miss += hit ? 0 : 1;
    }
    for (int e = lane; e < nb; e += 64) {
      const int2 w = s_inv[e];
      const int ti = pi + rd(w.x - su), tj = pj + rd(w.y - sv);
      bool hit = false;
      if ((unsigned)ti < (unsigned)G && (unsigned)tj < (unsigned)G) {
        const int idx = ti * G + tj;
        hit = (s_a[idx >> 5] >> (idx & 31)) & 1u;
      }
      miss += hit ? 0 : 1;
    }
    const int cost = wave_sum(miss);
    const unsigned long long key = motion_key(cost, si, sj, k, A, R);
    best = key < best ? key : best;
  }
  if (lane == 0 && best != ~0ull) atomicMin(s_key, best);
  __syncthreads();
  if (tid == 0 && *s_key != ~0ull) atomicMax(&keys[bp * MAX_A + k], ~*s_key);  // the least key is the largest complement
}

// ---- 3. the best records ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void answer_kernel(const int *__restrict__ heads, const unsigned long long *__restrict__ keys,
                                                    const long long *__restrict__ frame_a, const long long *__restrict__ frame_b, int A,
                                                    int R, int P, int *__restrict__ rot, int *__restrict__ best) {
  const int t = blockIdx.x, lane = threadIdx.x, b = t / P;
  const int *head = heads + (size_t)t * HEAD;
  const int na = head[H_NA], nb = head[H_NB];
  int status = 1;
  if (!common_frame(frame_a, frame_b, b)) status = 0;  // the gather added nothing: na = nb = 0
  else if (na == 0 || nb == 0) status = 2;
  else if (na > MAX_CELLS || nb > MAX_CELLS) status = 3;
  const bool live = status == 1 && lane < A;  // every search block of an evaluated pair wrote its key
  const unsigned long long stored = live ? keys[(size_t)t * MAX_A + lane] : 0ull, key = ~stored;
  const int side = 2 * R + 1, sidx = (int)(key & 2047ull);
  const int cost = live ? (int)(key >> 33) : -1, si = live ? sidx / side - R : 0, sj = live ? sidx - (sidx / side) * side - R : 0;
  int *row = rot + ((size_t)t * MAX_A + lane) * 4;
  row[0] = cost;
  row[1] = si;
  row[2] = sj;
  row[3] = 0;
  const unsigned long long top = ~wave_max64(stored);  // the least key over k
  const int k = (int)(top >> 11) & 63, d = abs(lane - k);
  const int far = wave_max(live && min(d, A - d) >= 2 ? (1 << 20) - cost : 0);  // cost <= 8192
  if (lane != 0) return;
  int out[UOC_MOTION_BEST_WORDS] = {status, -1, 0, 0, 0, na, nb, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (status == 1) {
    const int bidx = (int)(top & 2047ull), bi = bidx / side - R, bj = bidx - (bidx / side) * side - R;
    const int pi = pivot(head[H_IA], na), pj = pivot(head[H_JA], na), qi = pivot(head[H_IB], nb), qj = pivot(head[H_JB], nb);
    out[1] = k;
    out[2] = bi;
    out[3] = bj;
    out[4] = (int)(top >> 33);
    out[7] = na + nb - 2 * head[H_BOTH];
    out[8] = pi;
    out[9] = pj;
    out[10] = qi;
    out[11] = qj;
    out[12] = qi + bi - pi;
    out[13] = qj + bj - pj;
    out[14] = far ? (1 << 20) - far : -1;
  }
  int *o = best + (size_t)t * UOC_MOTION_BEST_WORDS;
#pragma unroll
  for (int w = 0; w < UOC_MOTION_BEST_WORDS; ++w) o[w] = out[w];
}

bool shape_ok(int B, int G, int A, int P) {
  return batch_ok(B) && grid_ok(G) && A >= 1 && A <= MAX_A && P >= 1 && P <= MAX_P;
}

struct Ws {
  int *heads;                // [B][P][8]
  unsigned long long *keys;  // [B][P][64]: the complement of the least key of rotation k, 0 while no block has written
  unsigned *lists;           // [B][P][2][4096]: (i << 16) | j
  size_t zero_bytes, total;  // heads and keys: zeroed per call
};
Ws carve(void *base, int B, int P) {
  Ws w;
  Carver cv(base);
  w.heads = cv.take<int>((size_t)B * P * HEAD);
  w.keys = cv.take<unsigned long long>((size_t)B * P * MAX_A);
  w.zero_bytes = cv.total();
  w.lists = cv.take<unsigned>((size_t)B * P * 2 * MAX_CELLS);
  w.total = cv.total();
  return w;
}

DeviceOnce g_search_lds;

}  // namespace
}  // namespace uoc

using namespace uoc;

extern "C" {

size_t uoc_motion_workspace_bytes(int B, int G, int A, int P) {
  if (!shape_ok(B, G, A, P)) return 0;
  return carve(nullptr, B, P).total;
}

int uoc_motion(const int32_t *d_state_a, const int32_t *d_owner_a, const int64_t *d_frame_a, const int32_t *d_state_b,
               const int32_t *d_owner_b, const int64_t *d_frame_b, int B, int G, const int32_t *h_rot, int A, int R,
               const int32_t *h_pairs, int P, int32_t *d_rot, int32_t *d_best, void *d_ws, size_t ws_bytes, void *stream) {
  UOC_REQUIRE(d_state_a && d_owner_a && d_state_b && d_owner_b && h_rot && h_pairs && d_rot && d_best && d_ws,
              "uoc_motion: null state / owner / rotations / pairs / rot / best / workspace");
  UOC_REQUIRE((d_frame_a == nullptr) == (d_frame_b == nullptr), "uoc_motion: one frame pointer is null and the other is not");
  UOC_REQUIRE(batch_ok(B), "uoc_motion: bad shape B=%d (B in 1..65535)", B);
  UOC_REQUIRE(grid_ok(G), "uoc_motion: grid = %d is not a multiple of 8 in [8, %d]", G, MAX_G);
  UOC_REQUIRE(A >= 1 && A <= MAX_A, "uoc_motion: %d rotations outside [1, %d]", A, MAX_A);
  UOC_REQUIRE(R >= 0 && R <= MAX_R, "uoc_motion: radius = %d outside [0, %d]", R, MAX_R);
  UOC_REQUIRE(P >= 1 && P <= MAX_P, "uoc_motion: %d pairs outside [1, %d]", P, MAX_P);
  Table table;
  for (int k = 0; k < MAX_A; ++k)
    for (int c = 0; c < 2; ++c) table.c[k][c] = k < A ? h_rot[k * 2 + c] : 0;
  for (int k = 0; k < A; ++k)
    UOC_REQUIRE(table.c[k][0] >= -SCALE && table.c[k][0] <= SCALE && table.c[k][1] >= -SCALE && table.c[k][1] <= SCALE,
                "uoc_motion: rotation %d = (%d, %d) has a word outside [-%d, %d]", k, table.c[k][0], table.c[k][1], SCALE, SCALE);
  Pairs pairs;
  for (int p = 0; p < MAX_P; ++p)
    for (int c = 0; c < 2; ++c) pairs.v[p][c] = p < P ? h_pairs[p * 2 + c] : 0;
  for (int p = 0; p < P; ++p)
    UOC_REQUIRE(pairs.v[p][0] >= 1 && pairs.v[p][0] < NUM_IDS && pairs.v[p][1] >= 1 && pairs.v[p][1] < NUM_IDS,
                "uoc_motion: pair %d = (%d, %d) has an id outside [1, 127]", p, pairs.v[p][0], pairs.v[p][1]);
  const Ws w = carve(d_ws, B, P);
  UOC_REQUIRE(ws_bytes >= w.total, "uoc_motion: workspace %zu < %zu bytes", ws_bytes, w.total);
  UOC_REQUIRE(aligned16(d_ws), "uoc_motion: workspace not 16-byte aligned");
  const int rc = opt_in_dynamic_lds((const void *)search_kernel, search_lds_bytes(MAX_G), g_search_lds);
  if (rc != UOC_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const long long *fa = (const long long *)d_frame_a, *fb = (const long long *)d_frame_b;
  // Few pairs and frames leave most of the machine idle: then the shifts of a rotation are shared among NS blocks.
  const int blocks = A * P * B, side = 2 * R + 1, per_block = (side * side + SEARCH_WAVES - 1) / SEARCH_WAVES;
  const int NS = blocks >= 1024 ? 1 : std::min(std::min(16, 1024 / blocks), per_block);
  UOC_HIP_CHECK(hipMemsetAsync(w.heads, 0, w.zero_bytes, st));
  hipLaunchKernelGGL(gather_kernel, dim3((G * G + GATHER_CHUNK - 1) / GATHER_CHUNK, P, B), dim3(GATHER_THREADS), 0, st, d_state_a,
                     d_owner_a, fa, d_state_b, d_owner_b, fb, G, P, pairs, w.heads, w.lists);
  hipLaunchKernelGGL(search_kernel, dim3(A * NS, P, B), dim3(SEARCH_THREADS), search_lds_bytes(G), st, w.heads, w.lists, G, A, R, P, NS,
                     table, w.keys);
  hipLaunchKernelGGL(answer_kernel, dim3(B * P), dim3(64), 0, st, w.heads, w.keys, fa, fb, A, R, P, d_rot, d_best);
  UOC_LAUNCH_CHECK();
  return UOC_OK;
}

}  // extern "C"
