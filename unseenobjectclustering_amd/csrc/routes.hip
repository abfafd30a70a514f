// Routes: reachability and slide paths on the table grid (include/uoc_hip.h, uoc_routes).
// From the state / owner grids and the frame records of uoc_placement and up to 8 query records (need2, si, sj, ti, tj,
// ignore, 0, 0): per query the field of least chamfer cost (5 per orthogonal, 7 per diagonal move, no corner cutting)
// from the source over the cells where a disc of squared radius need2 fits, the closest approach to the target and the
// path back from it.  Integers only.
//
// One memset (the sweep counters in the workspace) and three launches:
//   run_kernel    grid (rows, maps, frames), 4 waves.  A map belongs to one distinct (ignore, need2); queries with the
//                 same pair share it.  The row's FREE bits by ballot into LDS, then per cell the length of the run of FREE
//                 cells that ends there: 16-bit words (grid.h's run_kernel, which footprint.hip launches too).  A frame
//                 without a plane gets zeros.
//   pass_kernel   grid (chunks of 256 cells, maps, frames).  A row of the disc is one span |dj| <= h(di), h from the host
//                 as a kernel argument: the span of row i+di is free iff it lies in the grid and
//                 run[i+di][j+h] >= 2h+1.  One byte per cell: PASSABLE or not.
//   solve_kernel  grid (queries, frames), 16 waves: ONE workgroup owns the field of a (frame, query) from the first
//                 relaxation to the last path cell.  The field has a border of blocked cells (no bounds test in the inner
//                 loop) and an odd pitch in dwords (a wave that walks 64 rows side by side hits 64 banks).  Where it lives:
//                   32-bit words in LDS while (G+2) rows fit 152 KB (G <= 192);
//                   16-bit words in LDS up to G = 272 (the common G = 256: 130 KB).  A value above 65533 does not fit: the
//                   relaxation that would store one raises a flag instead, and at the end of that sweep the workgroup
//                   copies the field (every value in it is the length of a real path, or "infinite") into 32-bit words
//                   in the workspace and goes on there.  Exact for every input; an open tabletop never leaves LDS;
//                   32-bit words in the workspace (L2: 1 MB at G = 512) above that.
//                 A sweep: every thread walks a segment of a row there and back, a barrier, every thread walks a segment
//                 of a column down and up, a barrier that also gathers "something changed".  A walk keeps the 3x3
//                 neighbourhood in registers and reads three new words per cell; a cell is written by its walker alone.
//                 Values start at "infinite", only decrease and are each the length of a real path, so a stale read of
//                 a neighbour only delays; a sweep that changes nothing read the final field everywhere and relaxed every
//                 cell against all eight neighbours: the unique fixpoint.  At most G*G sweeps (twice that after the
//                 hand-over): no input can keep the loop going.
//                 Tail, same workgroup, the field still in place: cost out, the counts and the closest-approach key
//                 (shuffles, LDS atomics), then wave 0 walks back: lanes 0..7 test one neighbour each, the lowest set
//                 bit of the ballot is the first neighbour in the fixed order.
//
// Determinism: the fixpoint of the relaxation is unique, the key is a strict total order and the walk back follows a
// fixed order: nothing depends on the schedule.  Nothing of frame b depends on the other frames of the batch.
#include "grid.h"
#include "prof.h"

namespace uoc {
namespace {

constexpr int MAX_Q = UOC_ROUTES_MAX_QUERIES;
constexpr int MAX_NEED2 = UOC_ROUTES_MAX_NEED2;
constexpr int MAX_PATH = UOC_ROUTES_MAX_PATH;
constexpr int MAX_R = 63;            // di*di < 4096
constexpr int ROWS = 2 * MAX_R + 2;  // 127 rows of the disc, padded to 128 bytes
constexpr int THREADS = 256;
constexpr int SOLVE_THREADS = 1024;
constexpr int COST_MASK = (1 << 21) - 1, DA_MASK = (1 << 19) - 1;
constexpr int LDS_FIELD_BYTES = 152 * 1024;  // of the CU's 160 KB; the rest is for the few words beside the field
constexpr int W_ORTH = 5, W_DIAG = 7;
constexpr unsigned PACK_DI = 0xA094u, PACK_DJ = 0x8861u;  // 2 bits per move k: d + 1 of (-1,0) (0,-1) (0,1) (1,0) (-1,-1) (-1,1) (1,-1) (1,1)
enum { FIELD_LDS32 = 0, FIELD_LDS16 = 1, FIELD_GLOBAL = 2 };

static_assert(7ll * MAX_G * MAX_G <= COST_MASK, "a cost must fit 21 bits of the key");
static_assert(2 * (MAX_G - 1) * (MAX_G - 1) <= DA_MASK, "da must fit 19 bits of the key");
static_assert((MAX_R + 1) * (MAX_R + 1) >= MAX_NEED2 && MAX_R * MAX_R < MAX_NEED2, "the disc has rows -63..63");

struct Queries {
  int v[MAX_Q][8];  // need2, si, sj, ti, tj, ignore, 0, 0
};
struct Plan {
  int map[MAX_Q];     // the map of query q
  RunIgnore<MAX_Q> ignore;  // of map m
  int need2[MAX_Q];   // of map m
  signed char half[MAX_Q][ROWS];  // h of row di + 63 of map m's disc: |dj| <= h, -1 for an empty row
};

__host__ __device__ inline int pitch32(int G) { return (G + 2) | 1; }                // dwords: odd
__host__ __device__ inline int pitch16(int G) { return 2 * (((G + 3) >> 1) | 1); }   // halfwords: an odd number of dwords
int field_mode(int G) {
#ifdef UOC_ROUTES_GLOBAL_FIELD
  return FIELD_GLOBAL;  // the A/B build of DESIGN.md §19: the plain form
#else
  if ((size_t)(G + 2) * pitch32(G) * 4 <= (size_t)LDS_FIELD_BYTES) return FIELD_LDS32;
  if ((size_t)(G + 2) * pitch16(G) * 2 <= (size_t)LDS_FIELD_BYTES) return FIELD_LDS16;
  return FIELD_GLOBAL;
#endif
}

// ---- 2. PASSABLE ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void pass_kernel(const unsigned short *__restrict__ runs, int G, int NM, Plan p,
                                                       unsigned char *__restrict__ pass) {
  const int m = blockIdx.y, b = blockIdx.z, cells = G * G;
  const int idx = blockIdx.x * THREADS + threadIdx.x;
  const unsigned short *run = runs + ((size_t)b * NM + m) * cells;
  const bool in = idx < cells;
  const int i = idx / G, j = idx - i * G;
  bool ok = in && run[idx] != 0;
  const int need2 = p.need2[m];
  int rmax = -1;  // need2 == 0: no offset at all, PASSABLE = FREE
  while ((rmax + 1) * (rmax + 1) < need2) ++rmax;
  for (int di = -rmax; di <= rmax && __any(ok); ++di) {  // uniform bounds
    const int h = p.half[m][di + MAX_R];
    const int ii = i + di, j1 = j + h;
    const bool inside = ok && (unsigned)ii < (unsigned)G && j - h >= 0 && j1 < G;
    const int got = inside ? run[ii * G + j1] : 0;
    ok = inside && got >= 2 * h + 1;
  }
  if (in) pass[((size_t)b * NM + m) * cells + idx] = ok ? 1 : 0;
}

// ---- 3. the field -----------------------------------------------------------------------------------------------------
// Word-sized relaxed accesses: a neighbour's word is read while its walker may be writing it; either value will do.
template <typename T>
struct Field {
  T *p;
  static constexpr unsigned BLK = (unsigned)(T)~(T)0;  // not PASSABLE (the border included)
  static constexpr unsigned INF = BLK - 1;             // PASSABLE, not reached
  static constexpr unsigned MAXV = BLK - 2;            // the largest cost the word holds
  __device__ __forceinline__ unsigned ld(int e) const {
    return (unsigned)__hip_atomic_load(p + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __device__ __forceinline__ void st(int e, unsigned v) const {
    __hip_atomic_store(p + e, (T)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
};
using F32 = Field<unsigned>;
using F16 = Field<unsigned short>;

struct Shared {
  unsigned long long key;
  int flags[2];
  int reached, passable, steps, last;
};

// n cells from element e along `step`; `lat` is the stride across.  Returns 1: a word changed, 2: a value did not fit.
template <class F>
__device__ __forceinline__ int walk(const F f, int e, int step, int lat, int n) {
  int flags = 0;
  unsigned a0 = f.ld(e - lat - step), a1 = f.ld(e - lat);
  unsigned b0 = f.ld(e - step), b1 = f.ld(e);
  unsigned c0 = f.ld(e + lat - step), c1 = f.ld(e + lat);
  for (int k = 0; k < n; ++k, e += step) {
    const unsigned a2 = f.ld(e - lat + step), b2 = f.ld(e + step), c2 = f.ld(e + lat + step);
    if (b1 != F::BLK) {
      const unsigned cur = b1 == F::INF ? ~0u : b1;  // "infinite" is above every candidate, one that does not fit included
      unsigned best = cur;
      const bool pa = a1 != F::BLK, pc = c1 != F::BLK, p0 = b0 != F::BLK, p2 = b2 != F::BLK;
      if (a1 < F::INF) best = min(best, a1 + W_ORTH);
      if (c1 < F::INF) best = min(best, c1 + W_ORTH);
      if (b0 < F::INF) best = min(best, b0 + W_ORTH);
      if (b2 < F::INF) best = min(best, b2 + W_ORTH);
      if (a0 < F::INF && pa && p0) best = min(best, a0 + W_DIAG);  // a reached cell is PASSABLE; the two between: no corner cutting
      if (a2 < F::INF && pa && p2) best = min(best, a2 + W_DIAG);
      if (c0 < F::INF && pc && p0) best = min(best, c0 + W_DIAG);
      if (c2 < F::INF && pc && p2) best = min(best, c2 + W_DIAG);
      if (best < cur) {
        if (best > F::MAXV) {
          flags |= 2;
        } else {
          f.st(e, best);
          b1 = best;
          flags |= 1;
        }
      }
    }
    a0 = a1, a1 = a2, b0 = b1, b1 = b2, c0 = c1, c1 = c2;
  }
  return flags;
}

// Sweeps until nothing changes (0), a value does not fit (2 or 3) or the bound is hit (1).
template <class F>
__device__ int relax(const F f, int G, int pitch, Shared &s, int &sweeps) {
  const int tid = threadIdx.x;
  const int segs = min(G, max(1, SOLVE_THREADS / G)), seglen = (G + segs - 1) / segs;
  const int line = tid % G, seg = tid / G, start = seg * seglen;
  const int n = seg < segs ? min(seglen, G - start) : 0;  // G * segs <= 1024 threads walk
  const int bound = G * G;
  int fl = 1;
  for (int sweep = 0; sweep < bound; ++sweep) {
    fl = 0;
    if (n > 0) {
      const int e = (line + 1) * pitch + start + 1;  // along a row, there and back
      fl |= walk(f, e, 1, pitch, n);
      fl |= walk(f, e + n - 1, -1, pitch, n);
    }
    __syncthreads();  // a cell has one writer at a time
    if (n > 0) {
      const int e = (start + 1) * pitch + line + 1;  // along a column
      fl |= walk(f, e, pitch, 1, n);
      fl |= walk(f, e + (n - 1) * pitch, -pitch, 1, n);
    }
    if (fl) atomicOr(&s.flags[sweep & 1], fl);
    __syncthreads();
    fl = s.flags[sweep & 1];
    if (tid == 0) s.flags[(sweep + 1) & 1] = 0;  // written again only after the next sweep's first barrier
    ++sweeps;
    if (fl != 1) break;
  }
  return fl;
}

// cost, info and path of one (frame, query) from the converged field.
template <class F>
__device__ void tail(const F f, int G, int pitch, const int *q, bool src_ok, int max_path, Shared &s, int *__restrict__ cost,
                     int *__restrict__ info, int *__restrict__ path) {
  const int tid = threadIdx.x, lane = tid & 63, cells = G * G;
  const int si = q[1], sj = q[2], ti = q[3], tj = q[4];
  const bool target = ti >= 0;
  int reached = 0, passable = 0;
  unsigned long long key = 0ull;
  for (int idx = tid; idx < cells; idx += SOLVE_THREADS) {  // cells is a multiple of 64: whole waves
    const int i = idx / G, j = idx - i * G;
    const unsigned v = f.ld((i + 1) * pitch + j + 1);
    const bool re = v < F::INF;
    passable += v != F::BLK;
    reached += re;
    cost[idx] = re ? (int)v : -1;
    if (re && target) {
      const int da = (i - ti) * (i - ti) + (j - tj) * (j - tj);
      key = max(key, ((unsigned long long)(DA_MASK - da) << 39) | ((unsigned long long)(COST_MASK - (int)v) << 18) |
                         cell_key(idx));
    }
  }
  reached = wave_sum(reached), passable = wave_sum(passable), key = wave_max64(key);
  if (lane == 0) {
    if (reached) atomicAdd(&s.reached, reached);
    if (passable) atomicAdd(&s.passable, passable);
    if (key) atomicMax(&s.key, key);
  }
  __syncthreads();
  key = s.key;
  if (tid < 64) {  // wave 0 walks back
    int rec[8] = {src_ok ? 1 : 0, 0, -1, -1, 0, 0, s.reached, s.passable};
    int last = -1;
    if (key) {
      const int idx = key_cell(key);
      unsigned vc = (unsigned)(COST_MASK - (int)((key >> 18) & (unsigned long long)COST_MASK));
      const int ci = idx / G, cj = idx - ci * G;
      int i = ci, j = cj, steps = 0;
      if (lane == 0) path[0] = ci, path[1] = cj;
      const int k = lane & 7, di = (int)((PACK_DI >> (2 * k)) & 3u) - 1, dj = (int)((PACK_DJ >> (2 * k)) & 3u) - 1;
      const unsigned w = k < 4 ? W_ORTH : W_DIAG;
      for (int it = 0; it < cells && !(i == si && j == sj); ++it) {  // a path has fewer than G*G moves
        const int e = (i + 1) * pitch + j + 1;
        const unsigned vn = f.ld(e + di * pitch + dj);
        bool ok = lane < 8 && vn < F::INF && vn + w == vc;
        if (k >= 4) ok = ok && f.ld(e + di * pitch) != F::BLK && f.ld(e + dj) != F::BLK;
        const unsigned long long hit = __ballot(ok);
        if (!hit) break;  // cannot happen at the fixpoint
        const int kk = __ffsll((long long)hit) - 1;
        i += (int)((PACK_DI >> (2 * kk)) & 3u) - 1;
        j += (int)((PACK_DJ >> (2 * kk)) & 3u) - 1;
        vc -= kk < 4 ? W_ORTH : W_DIAG;
        ++steps;
        if (lane == 0 && steps < max_path) path[2 * steps] = i, path[2 * steps + 1] = j;
      }
      rec[1] = (ci == ti && cj == tj) ? 1 : 0;
      rec[2] = ci, rec[3] = cj;
      rec[4] = COST_MASK - (int)((key >> 18) & (unsigned long long)COST_MASK);
      rec[5] = steps;
      last = min(steps, max_path - 1);
    }
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 8; ++k) info[k] = rec[k];
      s.last = last;
    }
  }
  __syncthreads();
  for (int k = s.last + 1 + tid; k < max_path; k += SOLVE_THREADS) path[2 * k] = -1, path[2 * k + 1] = -1;
}

template <class F>
__device__ void fill(const F f, int G, int pitch, const unsigned char *__restrict__ pass, int src, bool src_ok) {
  const int side = G + 2;
  for (int e = threadIdx.x; e < side * side; e += SOLVE_THREADS) {
    const int r = e / side, c = e - r * side;
    const bool inside = r >= 1 && r <= G && c >= 1 && c <= G;
    const int idx = (r - 1) * G + c - 1;
    unsigned v = inside && pass[idx] ? F::INF : F::BLK;
    if (inside && idx == src && src_ok) v = 0u;
    f.st(r * pitch + c, v);
  }
}

__global__ __launch_bounds__(SOLVE_THREADS) void solve_kernel(const unsigned char *__restrict__ pass, int G, int NM, int Q, Queries qs,
                                                              Plan p, int mode, int max_path, unsigned *__restrict__ gfield,
                                                              int *__restrict__ sweeps_out, int *__restrict__ cost,
                                                              int *__restrict__ info, int *__restrict__ path) {
  extern __shared__ __align__(16) unsigned char s_field[];
  __shared__ Shared s;
  const int tid = threadIdx.x, q = blockIdx.x, b = blockIdx.y, cells = G * G;
  const size_t bq = (size_t)b * Q + q;
  const int *rec = qs.v[q];
  const int src = rec[1] * G + rec[2];
  pass += ((size_t)b * NM + p.map[q]) * cells;
  cost += bq * cells, info += bq * 8, path += bq * 2 * max_path;
  const bool src_ok = pass[src] != 0;  // uniform
  if (tid == 0) {
    s.key = 0ull;
    s.flags[0] = s.flags[1] = 0;
    s.reached = s.passable = s.steps = 0;
    s.last = -1;
  }
  const int p32 = pitch32(G), p16 = pitch16(G);
  const F32 g{gfield + bq * (size_t)(G + 2) * p32};
  int sweeps = 0;
  if (mode == FIELD_LDS32) {
    const F32 f{(unsigned *)s_field};
    fill(f, G, p32, pass, src, src_ok);
    __syncthreads();
    if (src_ok) relax(f, G, p32, s, sweeps);
    tail(f, G, p32, rec, src_ok, max_path, s, cost, info, path);
  } else if (mode == FIELD_LDS16) {
    const F16 f{(unsigned short *)s_field};
    fill(f, G, p16, pass, src, src_ok);
    __syncthreads();
    const int fl = src_ok ? relax(f, G, p16, s, sweeps) : 0;
    if (fl & 2) {  // uniform: a cost above 65533.  Every word is the length of a real path or "infinite": go on in 32 bits
      const int side = G + 2;
      for (int e = tid; e < side * side; e += SOLVE_THREADS) {
        const int r = e / side, c = e - r * side;
        const unsigned v = f.ld(r * p16 + c);
        g.st(r * p32 + c, v == F16::BLK ? F32::BLK : v == F16::INF ? F32::INF : v);
      }
      __syncthreads();  // every thread has read the flags of the last sweep
      if (tid == 0) s.flags[0] = s.flags[1] = 0;
      __syncthreads();
      relax(g, G, p32, s, sweeps);
      tail(g, G, p32, rec, src_ok, max_path, s, cost, info, path);
    } else {
      tail(f, G, p16, rec, src_ok, max_path, s, cost, info, path);
    }
  } else {
    fill(g, G, p32, pass, src, src_ok);
    __syncthreads();
    if (src_ok) relax(g, G, p32, s, sweeps);
    tail(g, G, p32, rec, src_ok, max_path, s, cost, info, path);
  }
  if (tid == 0) sweeps_out[bq] = sweeps;
}

bool shape_ok(int B, int G, int Q) {
  return batch_ok(B) && grid_ok(G) && Q >= 1 && Q <= MAX_Q;
}

struct Ws {
  int *sweeps;           // [B][Q]: the sweeps each (frame, query) took, a diagnostic
  unsigned short *runs;  // room for [B][Q][G][G]; a call packs its NM <= Q maps per frame: [B][NM][G][G]
  unsigned char *pass;   // likewise
  unsigned *field;       // [B][Q][G+2][pitch32] where the field of a workgroup may leave LDS
  size_t sweeps_bytes, total;
};
Ws carve(void *base, int B, int G, int Q) {
  Ws w;
  Carver cv(base);
  w.sweeps_bytes = (size_t)B * Q * sizeof(int);
  w.sweeps = cv.take<int>((size_t)B * Q);
  w.runs = cv.take<unsigned short>((size_t)B * Q * G * G);
  w.pass = cv.take<unsigned char>((size_t)B * Q * G * G);
  w.field = cv.take<unsigned>(field_mode(G) == FIELD_LDS32 ? 0 : (size_t)B * Q * (G + 2) * pitch32(G));
  w.total = cv.total();
  return w;
}

}  // namespace
}  // namespace uoc

using namespace uoc;

extern "C" {

size_t uoc_routes_workspace_bytes(int B, int G, int Q) {
  if (!shape_ok(B, G, Q)) return 0;
  return carve(nullptr, B, G, Q).total;
}

int uoc_routes(const int32_t *d_state, const int32_t *d_owner, const int64_t *d_frame, int B, int G, const int32_t *h_queries, int Q,
               int unknown_blocks, int max_path, int32_t *d_cost, int32_t *d_info, int32_t *d_path, void *d_ws, size_t ws_bytes,
               void *stream) {
  UOC_REQUIRE(d_state && d_owner && h_queries && d_cost && d_info && d_path && d_ws,
              "uoc_routes: null state / owner / queries / cost / info / path / workspace");
  UOC_REQUIRE(batch_ok(B), "uoc_routes: bad shape B=%d (B in 1..65535)", B);
  UOC_REQUIRE(grid_ok(G), "uoc_routes: grid = %d is not a multiple of 8 in [8, %d]", G, MAX_G);
  UOC_REQUIRE(Q >= 1 && Q <= MAX_Q, "uoc_routes: %d queries outside [1, %d]", Q, MAX_Q);
  UOC_REQUIRE(unknown_blocks == 0 || unknown_blocks == 1, "uoc_routes: unknown_blocks = %d is neither 0 nor 1", unknown_blocks);
  UOC_REQUIRE(max_path >= 1 && max_path <= MAX_PATH, "uoc_routes: max_path = %d outside [1, %d]", max_path, MAX_PATH);
  Queries qs;
  Plan p;
  int NM = 0;
  for (int q = 0; q < MAX_Q; ++q) {
    for (int k = 0; k < 8; ++k) qs.v[q][k] = q < Q ? h_queries[q * 8 + k] : 0;
    p.map[q] = p.ignore.v[q] = p.need2[q] = 0;
    for (int r = 0; r < ROWS; ++r) p.half[q][r] = -1;
  }
  for (int q = 0; q < Q; ++q) {
    const int *v = qs.v[q];
    UOC_REQUIRE(v[0] >= 0 && v[0] <= MAX_NEED2, "uoc_routes: query %d: need2 = %d outside [0, %d]", q, v[0], MAX_NEED2);
    UOC_REQUIRE(v[1] >= 0 && v[1] < G && v[2] >= 0 && v[2] < G, "uoc_routes: query %d: source (si, sj) = (%d, %d) outside the grid", q, v[1],
                v[2]);
    UOC_REQUIRE((v[3] == -1 && v[4] == -1) || (v[3] >= 0 && v[3] < G && v[4] >= 0 && v[4] < G),
                "uoc_routes: query %d: target (ti, tj) = (%d, %d) is neither inside the grid nor (-1, -1)", q, v[3], v[4]);
    UOC_REQUIRE(v[5] >= 0 && v[5] < NUM_IDS, "uoc_routes: query %d: ignore = %d outside [0, 127]", q, v[5]);
    UOC_REQUIRE(v[6] == 0 && v[7] == 0, "uoc_routes: query %d: reserved words (%d, %d) are not zero", q, v[6], v[7]);
    int m = 0;
    while (m < NM && !(p.ignore.v[m] == v[5] && p.need2[m] == v[0])) ++m;
    if (m == NM) {
      p.ignore.v[m] = v[5], p.need2[m] = v[0];
      for (int di = -MAX_R; di <= MAX_R; ++di) {  // the span of row di: dj*dj < need2 - di*di
        int h = -1;
        while ((h + 1) * (h + 1) < v[0] - di * di) ++h;
        p.half[m][di + MAX_R] = (signed char)h;
      }
      ++NM;
    }
    p.map[q] = m;
  }
  const Ws w = carve(d_ws, B, G, Q);
  UOC_REQUIRE(ws_bytes >= w.total, "uoc_routes: workspace %zu < %zu bytes", ws_bytes, w.total);
  UOC_REQUIRE(aligned16(d_ws), "uoc_routes: workspace not 16-byte aligned");
  const int cells = G * G, mode = field_mode(G);
  const size_t lds = mode == FIELD_LDS32 ? (size_t)(G + 2) * pitch32(G) * 4 : mode == FIELD_LDS16 ? (size_t)(G + 2) * pitch16(G) * 2 : 0;
  static DeviceOnce attr_set;
  if (int rc = opt_in_dynamic_lds(reinterpret_cast<const void *>(&solve_kernel), LDS_FIELD_BYTES, attr_set)) return rc;
  hipStream_t st = (hipStream_t)stream;
  {
    ProfScope prof(KC_ROUTES_TABLES, st, 0.0, (double)B * cells * (8.0 + 5.0 * NM));
    UOC_HIP_CHECK(hipMemsetAsync(w.sweeps, 0, w.sweeps_bytes, st));
    hipLaunchKernelGGL(run_kernel<MAX_Q>, dim3(G, NM, B), dim3(RUN_THREADS), 0, st, d_state, d_owner, (const long long *)d_frame, G,
                       NM, p.ignore, unknown_blocks, w.runs);
    hipLaunchKernelGGL(pass_kernel, dim3((cells + THREADS - 1) / THREADS, NM, B), dim3(THREADS), 0, st, w.runs, G, NM, p, w.pass);
  }
  {
    ProfScope prof(KC_ROUTES_SOLVE, st, 0.0, (double)B * Q * cells * 5.0);
    hipLaunchKernelGGL(solve_kernel, dim3(Q, B), dim3(SOLVE_THREADS), lds, st, w.pass, G, NM, Q, qs, p, mode, max_path, w.field, w.sweeps,
                       d_cost, d_info, d_path);
  }
  UOC_LAUNCH_CHECK();
  return UOC_OK;
}

}  // extern "C"
