// The table grid, once: what placement.hip, elevation.hip, grasp.hip, footprint.hip, routes.hip, normals.hip and
// scene.hip share.  The integer frame of a support plane and its 16-word record, the projection of a
// point into a cell, the pixel sweep of the raster passes, the per-wave combination of distinct cells, the two passes of
// the exact distance transform, the runs of FREE cells, the widest-cell key, the placement queries and the host-side
// shape checks.  Every stage that names a cell means the cell these functions give it.  Integers only; everything
// returns the same bits from run to run.
#pragma once
#include "labelmap.h"

#include <limits.h>
#include <math.h>

namespace uoc {

constexpr int SCALE = 16384;     // S: a unit vector's component in the frame, a direction's in the tables
constexpr int MAX_G = UOC_PLACE_MAX_GRID;       // cells per side
constexpr int IDX_MASK = 0x3FFFF;
constexpr int MAX_ANCHOR = UOC_PLACE_MAX_ANCHOR;
constexpr int PIX_WAVES = 4;             // the pixel sweep: waves per block,
constexpr int PIX_SUB = 1024;            // pixels per wave,
constexpr int PIX_CHUNK = PIX_WAVES * PIX_SUB;   // pixels per block
constexpr int STRIP = 32;        // columns per block of the column pass
constexpr int SEGS = 8;          // row segments per column: STRIP * SEGS threads
constexpr int ROW_THREADS = 256;
constexpr int RUN_THREADS = 256;

// The frame record: 16 int64 words per frame.
constexpr int NFR = 16;
constexpr int FR_N = 0, FR_D = 3, FR_U = 4, FR_V = 7, FR_QC = 10, FR_FOUND = 13, FR_ZERO = 14;  // N, U, V, qc: three words each

static_assert(MAX_G * MAX_G <= IDX_MASK + 1, "a cell index must fit the key's low 18 bits");
static_assert((MAX_G / 2) * (MAX_G / 2) < (1 << 17), "dist2 must fit 17 bits of the key");
static_assert(2ll * (MAX_ANCHOR + MAX_G) * (MAX_ANCHOR + MAX_G) < (1ll << 26), "an anchor distance stays below 2^26");
static_assert(STRIP * SEGS == 256 && MAX_G % SEGS == 0, "column pass layout");
static_assert(MAX_G <= 65535 && MAX_G / 64 <= 8, "a run is one 16-bit word, a row at most 8 ballot words");
static_assert(sizeof(uoc_plane) == 21 * 4, "uoc_plane is 21 words");
static_assert(FR_FOUND + 1 == FR_ZERO && FR_ZERO + 2 == NFR, "the record ends with found and two zero words");

// ---- the frame --------------------------------------------------------------------------------------------------------
struct Frame {
  int N[3], U[3], V[3], qc[3];
  long long D;
  int found;
};

__device__ __forceinline__ bool frame_unit_ok(float a) { return isfinite(a) && fabsf(a) <= 2.0f; }
__device__ __forceinline__ bool frame_within(long long v, long long lim) { return v >= -lim && v <= lim; }

// Step F: a plane record into the integer frame, all zero when the record cannot be used.  Wave-uniform: every thread
// reads the same record.
__device__ __forceinline__ Frame frame_from_plane(const uoc_plane &p) {
  Frame f;
  f.found = 0;
  f.D = 0;
  for (int k = 0; k < 3; ++k) f.N[k] = f.U[k] = f.V[k] = f.qc[k] = 0;
  bool ok = p.found == 1 && isfinite(p.d) && fabsf(p.d) <= 1000.0f;
  float r[3];
  for (int k = 0; k < 3; ++k) {
    ok = ok && frame_unit_ok(p.normal[k]) && frame_unit_ok(p.u[k]) && frame_unit_ok(p.v[k]) && isfinite(p.centroid[k]);
    r[k] = rintf(p.centroid[k] * 1000.0f);
    ok = ok && fabsf(r[k]) <= 32767.0f;
  }
  if (ok) {
    for (int k = 0; k < 3; ++k) {
      f.N[k] = (int)rint((double)p.normal[k] * 16384.0);
      f.U[k] = (int)rint((double)p.u[k] * 16384.0);
      f.V[k] = (int)rint((double)p.v[k] * 16384.0);
      f.qc[k] = (int)r[k];
    }
    f.D = (long long)rint((double)p.d * 16384000.0);
    f.found = 1;
  }
  return f;
}

__device__ __forceinline__ void store_frame(long long *__restrict__ F, const Frame &f) {
  for (int k = 0; k < 3; ++k) {
    F[FR_N + k] = f.N[k];
    F[FR_U + k] = f.U[k];
    F[FR_V + k] = f.V[k];
    F[FR_QC + k] = f.qc[k];
  }
  F[FR_D] = f.D;
  F[FR_FOUND] = f.found;
  F[FR_ZERO] = F[FR_ZERO + 1] = 0;
}

// "This frame has a plane", three ways.  They agree on every record store_frame wrote and differ on a caller's own:
//   frame_found_nonzero      the found word is not 0                          (placement's column pass)
//   frame_found_one_or_null  the found word is 1, or there are no records     (the runs of footprint and routes)
//   load_frame(F).found      the found word is 1 and every word is in range   (elevation)
__device__ __forceinline__ bool frame_found_nonzero(const long long *__restrict__ F) { return F[FR_FOUND] != 0; }
__device__ __forceinline__ bool frame_found_one_or_null(const long long *__restrict__ frame, int b) {
  return frame == nullptr || frame[(size_t)b * NFR + FR_FOUND] == 1;
}
__device__ __forceinline__ Frame load_frame(const long long *__restrict__ F) {
  Frame f;
  bool ok = F[FR_FOUND] == 1 && frame_within(F[FR_D], 1ll << 34);
  for (int k = 0; k < 3; ++k)
    ok = ok && frame_within(F[FR_N + k], 32768) && frame_within(F[FR_U + k], 32768) && frame_within(F[FR_V + k], 32768) && frame_within(F[FR_QC + k], 32767);
  for (int k = 0; k < 3; ++k) {
    f.N[k] = ok ? (int)F[FR_N + k] : 0;
    f.U[k] = ok ? (int)F[FR_U + k] : 0;
    f.V[k] = ok ? (int)F[FR_V + k] : 0;
    f.qc[k] = ok ? (int)F[FR_QC + k] : 0;
  }
  f.D = ok ? F[FR_D] : 0;
  f.found = ok ? 1 : 0;
  return f;
}

// ---- a point into a cell ----------------------------------------------------------------------------------------------
__device__ __forceinline__ long long floor_div(long long a, int c) {  // c > 0
  const long long q = a / c;
  return q - ((a - q * c) < 0 ? 1 : 0);
}

// Step P.  cell_div = cell_mm * S, t_low = -tau_mm * S.  A point is ignored (not valid, or more than tau below the
// plane), outside the grid (the function returns true) or inside: then `inside(i, j, T)` gets its cell and its height
// above the plane in units of 1/S mm.  The tests in this order: validity, the grid, the height.
template <typename Inside>
__device__ __forceinline__ bool project_point(const Frame &f, int cell_div, int t_low, int G, float x, float y, float z,
                                              Inside inside) {
  if (!(isfinite(x) && isfinite(y) && isfinite(z) && z > 0.f)) return false;
  const float rx = rintf(x * 1000.0f), ry = rintf(y * 1000.0f), rz = rintf(z * 1000.0f);
  if (!(fabsf(rx) <= 32767.f && fabsf(ry) <= 32767.f && fabsf(rz) <= 32767.f)) return false;
  const int qx = (int)rx, qy = (int)ry, qz = (int)rz;
  const int dx = qx - f.qc[0], dy = qy - f.qc[1], dz = qz - f.qc[2];
  const long long A = (long long)f.U[0] * dx + (long long)f.U[1] * dy + (long long)f.U[2] * dz;
  const long long Bv = (long long)f.V[0] * dx + (long long)f.V[1] * dy + (long long)f.V[2] * dz;
  const long long i = floor_div(A, cell_div) + G / 2, j = floor_div(Bv, cell_div) + G / 2;
  if ((unsigned long long)i >= (unsigned long long)G || (unsigned long long)j >= (unsigned long long)G) return true;
  const long long T = (long long)f.N[0] * qx + (long long)f.N[1] * qy + (long long)f.N[2] * qz + f.D;
  if (T < t_low) return false;
  inside((int)i, (int)j, T);
  return false;
}

// ---- the pixel sweep --------------------------------------------------------------------------------------------------
template <int K>
struct Pixels {
  int l[K];
  float x[K], y[K], z[K];  // z = 0 past the end of the frame: no point
};

// The pixel sweep of a kernel launched on (pixel chunks of PIX_CHUNK, frames) with PIX_WAVES waves: a wave owns PIX_SUB
// consecutive pixels of the frame's n, a lane K = 4 consecutive ones per turn (one int4 and three float4 loads; n a
// multiple of 4, L and X 16-byte aligned) or K = 1.  `for (PixelSweep<VEC> s(L, X, n); s.load(px);) ...`: every lane of a
// wave takes the same number of turns, so the body may ballot and shuffle.
template <bool VEC>
struct PixelSweep {
  static constexpr int K = VEC ? 4 : 1;
  const int *__restrict__ L;
  const float *__restrict__ X;
  long long n, base;
  int it = 0;
  __device__ __forceinline__ PixelSweep(const int *__restrict__ L_, const float *__restrict__ X_, long long n_)
      : L(L_), X(X_), n(n_), base((long long)blockIdx.x * PIX_CHUNK + (long long)(threadIdx.x >> 6) * PIX_SUB) {}
  __device__ __forceinline__ bool load(Pixels<K> &px) {
    if (it >= PIX_SUB / (64 * K) || base >= n) return false;  // uniform per wave
    const long long p = base + (long long)(threadIdx.x & 63) * K;
    if constexpr (VEC) {
      int4 l4 = make_int4(0, 0, 0, 0);
      float4 x4 = make_float4(0.f, 0.f, 0.f, 0.f), y4 = x4, z4 = x4;
      if (p < n) {  // n is a multiple of 4: the four pixels are inside together
        l4 = *reinterpret_cast<const int4 *>(L + p);
        x4 = *reinterpret_cast<const float4 *>(X + p);
        y4 = *reinterpret_cast<const float4 *>(X + n + p);
        z4 = *reinterpret_cast<const float4 *>(X + 2 * n + p);
      }
      px = {{l4.x, l4.y, l4.z, l4.w}, {x4.x, x4.y, x4.z, x4.w}, {y4.x, y4.y, y4.z, y4.w}, {z4.x, z4.y, z4.z, z4.w}};
    } else {
      px = {{0}, {0.f}, {0.f}, {0.f}};
      if (p < n) px = {{L[p]}, {X[p]}, {X[n + p]}, {X[2 * n + p]}};
    }
    ++it;
    base += 64 * K;
    return true;
  }
};

// The (lane, slot) places of the wave whose flag is set.
template <int K>
__device__ __forceinline__ int wave_count_set(const bool (&flag)[K]) {
  int total = 0;
#pragma unroll
  for (int k = 0; k < K; ++k) total += __popcll(__ballot(flag[k]));
  return total;
}

// Every distinct code >= 0 among the K slots of the wave's lanes is handed to `emit` once, by one lane, with the number
// of (lane, slot) places that hold it and, with MAXW, the largest of their values w.  Every lane of the wave must call
// this.
template <int K, bool MAXW, typename Emit>
__device__ __forceinline__ void wave_distinct(int (&e)[K], const int (&w)[K], int lane, Emit emit) {
#pragma unroll
  for (int j = 0; j < K; ++j) {
    for_each_wave_key(e[j], [&](int c, unsigned long long m, int first) {
      int total = __popcll(m), mine = 0;
#pragma unroll
      for (int k = j; k < K; ++k) {
        const bool hit = e[k] == c;
        if (k > j) total += __popcll(__ballot(hit));
        if (hit) {
          if (k > j) e[k] = -1;  // slot j's own turns are the primitive's to count off
          mine = max(mine, w[k]);
        }
      }
      if constexpr (MAXW) mine = wave_max(mine);
      if (lane == first) emit(c, total, mine);
    });
  }
}

// ---- the distance transform -------------------------------------------------------------------------------------------
// The column pass of a block of STRIP * SEGS threads on the strip of columns from j0.  s[i][jj] holds bit 15 for a
// blocking cell (written by the block, a barrier since); g_out, the frame's [G][G] words, gets the distance along i to
// the nearest blocking cell of the column, the virtual cells at i = -1 and i = G included: 8 row segments per column
// scanned up and down, the carry between segments through LDS.
__device__ __forceinline__ void column_scan(unsigned short (&s)[MAX_G][STRIP], int G, int j0, int *__restrict__ g_out) {
  __shared__ int s_first[SEGS][STRIP], s_last[SEGS][STRIP];
  const int tid = threadIdx.x;
  const int jj = tid % STRIP, seg = tid / STRIP, rows = G / SEGS, r0 = seg * rows, r1 = r0 + rows;
  const bool col = j0 + jj < G;
  {  // the first and the last blocking row of the segment
    int first = INT_MAX, last = -1;
    if (col)
      for (int i = r0; i < r1; ++i)
        if (s[i][jj] & 0x8000u) {
          if (first == INT_MAX) first = i;
          last = i;
        }
    s_first[seg][jj] = first;
    s_last[seg][jj] = last;
  }
  __syncthreads();
  if (!col) return;
  int up = -1, down = G;  // the virtual blocking cells
  for (int k = seg - 1; k >= 0; --k)
    if (s_last[k][jj] >= 0) {
      up = s_last[k][jj];
      break;
    }
  for (int k = seg + 1; k < SEGS; ++k)
    if (s_first[k][jj] != INT_MAX) {
      down = s_first[k][jj];
      break;
    }
  for (int i = r0; i < r1; ++i) {  // distance up, at most 512: bits 0..9
    const unsigned v = s[i][jj];
    if (v & 0x8000u) up = i;
    s[i][jj] = (unsigned short)((v & 0x8000u) | (unsigned)(i - up));
  }
  for (int i = r1 - 1; i >= r0; --i) {
    const unsigned v = s[i][jj];
    if (v & 0x8000u) down = i;
    g_out[(size_t)i * G + j0 + jj] = min((int)(v & 0x7FFFu), down - i);
  }
}

// The row pass of a block of ROW_THREADS threads on one row of G words: g, as the column pass left it, squared into
// s_g2 (16-byte aligned, MAX_G words; a barrier before row_min_dist2), then per column j the minimum over j' of
// (j - j')^2 + g[j']^2 with the virtual columns at -1 and G.  Every lane reads the same words: a broadcast.
__device__ __forceinline__ void row_fill_g2(int *__restrict__ s_g2, const int *__restrict__ g, int G) {
  for (int j = threadIdx.x; j < G; j += ROW_THREADS) {
    const int v = g[j];
    s_g2[j] = v * v;
  }
}
__device__ __forceinline__ int row_min_dist2(const int *__restrict__ s_g2, int j, int G) {
  int best = min((j + 1) * (j + 1), (G - j) * (G - j));  // the virtual columns -1 and G
  for (int k = 0; k < G; k += 4) {                       // G is a multiple of 8
    const int4 v = *reinterpret_cast<const int4 *>(&s_g2[k]);
    const int d = j - k;
    best = min(best, d * d + v.x);
    best = min(best, (d - 1) * (d - 1) + v.y);
    best = min(best, (d - 2) * (d - 2) + v.z);
    best = min(best, (d - 3) * (d - 3) + v.w);
  }
  return best;
}

// ---- the keys ---------------------------------------------------------------------------------------------------------
// A cell index as the low 18 bits of a key: among equal keys above it the lowest cell wins a maximum.  The widest-cell
// key (0: no candidate), dist2 <= (G/2)^2 = 2^16:  ((dist2 + 1) << 18) | (0x3FFFF - idx).
__device__ __forceinline__ unsigned long long cell_key(int idx) { return (unsigned long long)(IDX_MASK - idx); }
__device__ __forceinline__ int key_cell(unsigned long long key) { return IDX_MASK - (int)(key & (unsigned long long)IDX_MASK); }
__device__ __forceinline__ unsigned long long widest_key(int dist2, int idx) {
  return ((unsigned long long)(dist2 + 1) << 18) | cell_key(idx);
}
__device__ __forceinline__ int key_dist2(unsigned long long key) { return (int)(key >> 18) - 1; }

// ---- the placement queries --------------------------------------------------------------------------------------------
// Rule Q of uoc_placement, for every stage that answers it on a state grid (placement.hip, scene.hip).  Keys (0: no
// candidate).  dist2 <= (G/2)^2 = 2^16, idx = i*G + j < 2^18, da = (i-ai)^2 + (j-aj)^2 <= 2 * (4096 + 511)^2 < 2^26:
//   widest   ((dist2 + 1) << 18) | (0x3FFFF - idx)
//   nearest  ((2^27 - 1 - da) << 35) | (dist2 << 18) | (0x3FFFF - idx)      for the candidates with dist2 >= need2
constexpr int PLACE_MAX_Q = UOC_PLACE_MAX_QUERIES;

static_assert(2ll * (MAX_ANCHOR + MAX_G) * (MAX_ANCHOR + MAX_G) < (1ll << 27) - 1, "the anchor distance must fit 27 bits");

struct PlaceQueries {
  int v[PLACE_MAX_Q][4];  // need2, ai, aj, mode
};

// The row pass with the query keys, the body of a kernel on grid (rows, frames) with ROW_THREADS threads: dist2 holds g
// as the column pass left it and gets the squared distance in place; per query one 64-bit key per candidate cell (state
// 1), the maximum per wave by shuffles, per block through LDS, per frame by atomicMax into keys [B][PLACE_MAX_Q] (zeroed).
__device__ __forceinline__ void row_pass_and_keys(const int *__restrict__ state, int G, const PlaceQueries &qs, int Q,
                                                  int *__restrict__ dist2, unsigned long long *__restrict__ keys) {
  __shared__ __attribute__((aligned(16))) int s_g2[MAX_G];
  __shared__ unsigned long long s_key[PLACE_MAX_Q];
  const int tid = threadIdx.x, lane = tid & 63, i = blockIdx.x, b = blockIdx.y;
  const size_t off = ((size_t)b * G + i) * G;
  row_fill_g2(s_g2, dist2 + off, G);
  if (tid < PLACE_MAX_Q) s_key[tid] = 0ull;
  __syncthreads();
  unsigned long long key[PLACE_MAX_Q];
#pragma unroll
  for (int q = 0; q < PLACE_MAX_Q; ++q) key[q] = 0ull;
  for (int j = tid; j < G; j += ROW_THREADS) {
    const int best = row_min_dist2(s_g2, j, G);
    dist2[off + j] = best;
    if (Q > 0 && state[off + j] == 1) {
      const unsigned long long low = cell_key(i * G + j);
#pragma unroll
      for (int q = 0; q < PLACE_MAX_Q; ++q) {
        unsigned long long k64 = 0ull;
        if (q >= Q) {  // uniform
        } else if (qs.v[q][3] == UOC_PLACE_WIDEST) {
          k64 = widest_key(best, i * G + j);
        } else if (best >= qs.v[q][0]) {
          const int di = i - qs.v[q][1], dj = j - qs.v[q][2];
          const unsigned long long da = (unsigned long long)(di * di + dj * dj);
          k64 = (((1ull << 27) - 1ull - da) << 35) | ((unsigned long long)best << 18) | low;
        }
        key[q] = max(key[q], k64);
      }
    }
  }
  if (Q == 0) return;
#pragma unroll
  for (int q = 0; q < PLACE_MAX_Q; ++q) {
    if (q < Q) {  // uniform
      const unsigned long long k64 = wave_max64(key[q]);
      if (lane == 0 && k64) atomicMax(&s_key[q], k64);
    }
  }
  __syncthreads();
  if (tid < Q && s_key[tid]) atomicMax(&keys[(size_t)b * PLACE_MAX_Q + tid], s_key[tid]);
}

// The keys back into (i, j, dist2, ok), the body of a kernel of one block per frame with at least PLACE_MAX_Q threads.
__device__ __forceinline__ void answer_queries(const unsigned long long *__restrict__ keys, int G, const PlaceQueries &qs, int Q,
                                               int *__restrict__ answers) {
  const int q = threadIdx.x, b = blockIdx.x;
  if (q >= Q) return;
  const unsigned long long k64 = keys[(size_t)b * PLACE_MAX_Q + q];
  int4 a = make_int4(-1, -1, 0, 0);
  if (k64) {
    const int idx = key_cell(k64);
    a.x = idx / G;
    a.y = idx % G;
    if (qs.v[q][3] == UOC_PLACE_WIDEST) {
      a.z = key_dist2(k64);
      a.w = a.z >= qs.v[q][0];
    } else {
      a.z = (int)((k64 >> 18) & 0x1FFFFull);
      a.w = 1;
    }
  }
  int *A = answers + ((size_t)b * Q + q) * 4;
  A[0] = a.x;
  A[1] = a.y;
  A[2] = a.z;
  A[3] = a.w;
}

// ---- the runs of FREE cells -------------------------------------------------------------------------------------------
template <int TABLES>
struct RunIgnore {
  int v[TABLES];  // the id that does not block in table t; 0 matches no id
};

// grid (rows, tables, frames), RUN_THREADS threads.  FREE: table, unknown unless unknown_blocks, or an obstacle of the
// table's `ignore`.  The row's FREE bits by ballot into LDS (8 words of 64 at G = 512), then per cell the length of the
// run of FREE cells that ends there, by counting leading ones: 16-bit words.  A frame without a plane gets zeros.
// Internal linkage: each stage that launches it gets a kernel of its own, as before.
namespace {
template <int TABLES>
__global__ __launch_bounds__(RUN_THREADS) void run_kernel(const int *__restrict__ state, const int *__restrict__ owner,
                                                          const long long *__restrict__ frame, int G, int NT, RunIgnore<TABLES> ig,
                                                          int unknown_blocks, unsigned short *__restrict__ runs) {
  __shared__ unsigned long long s_bits[MAX_G / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = blockIdx.x, t = blockIdx.y, b = blockIdx.z;
  const bool found = frame_found_one_or_null(frame, b);  // uniform per frame
  const int ignore = ig.v[t];
  const size_t in = ((size_t)b * G + i) * G, out = (((size_t)b * NT + t) * G + i) * G;
  for (int jb = 0; jb < G; jb += RUN_THREADS) {  // uniform: every lane takes part in the ballot
    const int j = jb + tid;
    bool fr = false;
    if (found && j < G) {
      const int st = state[in + j];
      if (st == 1) {
        fr = true;
      } else if (st == 2) {
        const int o = owner[in + j];
        fr = obj_id(o) ? (o == ignore) : !unknown_blocks;  // ignore == 0 matches no id
      } else {
        fr = !unknown_blocks;  // state 0 and every state outside 0..2: unknown
      }
    }
    const unsigned long long m = __ballot(fr);
    if (lane == 0 && jb + wave * 64 < G) s_bits[(jb >> 6) + wave] = m;
  }
  __syncthreads();
  for (int j = tid; j < G; j += RUN_THREADS) {
    int w = j >> 6, len = 0;
    unsigned long long x = ~s_bits[w] << (63 - (j & 63));  // bit 63 is cell j; a set bit is a cell that is not FREE
    while (true) {
      if (x) {
        len += __clzll((long long)x);
        break;
      }
      len += (w == (j >> 6)) ? (j & 63) + 1 : 64;
      if (--w < 0) break;
      x = ~s_bits[w];
    }
    runs[out + j] = (unsigned short)len;
  }
}
}  // namespace

// ---- the host side ----------------------------------------------------------------------------------------------------
inline bool grid_ok(int G) { return G >= 8 && G <= MAX_G && G % 8 == 0; }
inline bool batch_ok(int B) { return B > 0 && B <= 65535; }
inline bool image_ok(int B, int H, int W) { return batch_ok(B) && H > 0 && W > 0 && (long long)H * W <= INT_MAX; }
inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// The host table of Q placement queries into qs, the rest zero; UOC_EINVAL in `who`'s name for a Q, a pointer or a
// word out of range.
inline int load_place_queries(const char *who, const int32_t *h_queries, const void *d_answers, int Q, PlaceQueries &qs) {
  UOC_REQUIRE(Q >= 0 && Q <= PLACE_MAX_Q, "%s: %d queries outside [0, %d]", who, Q, PLACE_MAX_Q);
  UOC_REQUIRE(Q == 0 || (h_queries && d_answers), "%s: null queries / answers with Q = %d", who, Q);
  for (int q = 0; q < PLACE_MAX_Q; ++q)
    for (int k = 0; k < 4; ++k) qs.v[q][k] = q < Q ? h_queries[q * 4 + k] : 0;
  for (int q = 0; q < Q; ++q) {
    UOC_REQUIRE(qs.v[q][0] >= 0 && qs.v[q][0] <= (1 << 30), "%s: query %d: need2 = %d outside [0, 2^30]", who, q, qs.v[q][0]);
    UOC_REQUIRE(qs.v[q][1] >= -MAX_ANCHOR && qs.v[q][1] < MAX_ANCHOR && qs.v[q][2] >= -MAX_ANCHOR && qs.v[q][2] < MAX_ANCHOR,
                "%s: query %d: anchor (%d, %d) outside [-4096, 4095]", who, q, qs.v[q][1], qs.v[q][2]);
    UOC_REQUIRE(qs.v[q][3] == UOC_PLACE_WIDEST || qs.v[q][3] == UOC_PLACE_NEAREST, "%s: query %d: mode = %d", who, q, qs.v[q][3]);
  }
  return UOC_OK;
}

}  // namespace uoc
