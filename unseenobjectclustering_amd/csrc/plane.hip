// Support plane of a frame's background and object heights above it (include/uoc_hip.h, uoc_support_plane;
// DESIGN.md §13).
//
// Input per frame b: labels [H][W] int32 (ids 1..127 are objects, anything else is background) and the XYZ planes
// [3][H][W] fp32 metres.  A candidate is a background pixel with finite x, y, z, z > 0 and millimetre coordinates
// q = rint(1000 p) inside int16.
//
// Launches (grid (chunk, frame) for the pixel passes, one block per frame otherwise):
//   memset              zero the scores, the object counts and the extent keys
//   cand_count_kernel   candidates per wave (a wave owns 1024 consecutive pixels)
//   cand_scan_kernel    exclusive scan of the wave counts -> raster-order rank bases, M
//   cand_scatter_kernel q of every candidate at its raster-order rank (int16 x 3, packed in 8 bytes)
//   hyp_kernel          per hypothesis: three hashed candidates -> n', c0 = tau*L - n'.p0, 2*tau*L   (int64)
//   score_kernel        per tile of 1024 candidates: 4 candidates per lane in registers against every hypothesis (read
//                       through the scalar cache), inliers counted by ballot, one integer atomic per (block, hypothesis)
//   pselect_kernel      argmax over the key ((score + 1) << 10) | (1023 - h)
//   plane_sum_kernel    fp64 sums of the winner's inliers per chunk
//   plane_mom_kernel    centroid (chunk order), centred second moments per chunk
//   pfit_kernel         covariance, cyclic Jacobi, normal / d / u / v, the uoc_plane record
//   obj_sum_kernel      per id: valid count, min / max height (ordered 64-bit keys), sums of the in-plane coordinates;
//                       the height map
//   obj_mean_kernel     foot points (chunk order)
//   obj_mom_kernel      centred 2x2 moments per chunk
//   obj_axis_kernel     2x2 eigen-solve, the records but for the box
//   obj_extent_kernel   min / max along the major and minor axis
//   obj_box_kernel      half extents and centre of the upright box
//
// uoc_support_planes is the same pipeline with (frame, plane) as the batch; uoc_support_plane is its
// K = 1 with no stop rule and no index map.  It repeats hyp / score / pselect on what the earlier planes left (pselect's
// stop rule and the removal band of the winner), recount_kernel / rescatter_kernel (the survivors, re-compacted in
// raster order between two 8-byte lists), then index_kernel (the first plane whose removal band holds a pixel claims
// it), plane_sum_kernel / plane_mom_kernel / pfit_kernel (the same refinement, its pixels taken from the index map
// instead of the winner's band), pextent_kernel, pinfo_kernel and the six object kernels.
//
// Determinism: steps A and B are integer arithmetic and integer atomic adds, which commute.  Every floating-point sum
// has a fixed order: a lane adds its own pixels in program order, a wave sums its lanes with a fixed DPP tree, a block
// adds its four waves in wave order, the per-frame kernels add the chunks in chunk order.  No float atomics; min / max
// go through order-preserving integer keys.  Nothing of frame b depends on the other frames of the batch (the hash does
// not see b), so its outputs are the same bits alone or in a batch.
#include "common.h"
#include "fixed_order.h"
#include "prof.h"

#include <limits.h>
#include <math.h>

namespace uoc {
namespace {

constexpr int NL = 128;             // ids 0..127; 1..127 are objects
constexpr int WAVES = 4;            // waves per block
constexpr int SUB = 1024;           // pixels per wave: a wave owns a contiguous sub-chunk (16 iterations of 64 pixels)
constexpr int CHUNK = WAVES * SUB;  // pixels per block
constexpr int TC = 4;               // candidates per lane of the scoring kernel
constexpr int TILE = 256 * TC;      // candidates per block of the scoring kernel
constexpr int MAX_HYP = UOC_PLANE_MAX_HYP;
constexpr int NFR = 16;             // doubles of a frame's refined plane: normal, d, centroid, u, v, found
enum { FR_N = 0, FR_D = 3, FR_C = 4, FR_U = 7, FR_V = 10, FR_FOUND = 13 };
enum { K_TMAX = 0, K_TMIN = 1, K_E0 = 2, NKEY = 6 };  // max key(t), max key(-t), then max / min along e and e'

// One hypothesis, ready for scoring: q is an inlier when 0 <= c0 + n.q <= thr2, that is |n.(q - p0)| <= tau*L.
struct Hyp {
  int nx, ny, nz;
  int ok;                   // 0: degenerate (n' = 0), scores -1
  long long c0;             // tau*L - n.p0
  unsigned long long thr2;  // 2*tau*L
};
struct PWin {  // winner of (frame, round)
  int found, hyp, score, M;
  Hyp h;   // inlier band:  |n'.(q - p0)| <= tau * L
  Hyp hr;  // removal band: |n'.(q - p0)| <= rem * L
};

__device__ __forceinline__ bool inlier(const Hyp &h, int qx, int qy, int qz) {
  const long long acc = h.c0 + (long long)h.nx * qx + (long long)h.ny * qy + (long long)h.nz * qz;
  return (unsigned long long)acc <= h.thr2;
}

struct Pt {
  int l;       // object id, or -1 for background / out of range
  bool point;  // finite x, y, z with z > 0
  bool cand;   // plane candidate
  float x, y, z;
  int qx, qy, qz;
};
__device__ __forceinline__ Pt load_pt(const int *__restrict__ L, const float *__restrict__ X, int n, int p) {
  Pt q{-1, false, false, 0.f, 0.f, 0.f, 0, 0, 0};
  if (p < n) {
    const int l = L[p];
    q.x = X[p];
    q.y = X[(size_t)n + p];
    q.z = X[2 * (size_t)n + p];
    q.point = isfinite(q.x) && isfinite(q.y) && isfinite(q.z) && q.z > 0.f;
    if (l >= 1 && l < NL) {
      q.l = l;
    } else if (q.point) {
      const float rx = rintf(q.x * 1000.0f), ry = rintf(q.y * 1000.0f), rz = rintf(q.z * 1000.0f);
      if (fabsf(rx) <= 32767.f && fabsf(ry) <= 32767.f && fabsf(rz) <= 32767.f) {
        q.cand = true;
        q.qx = (int)rx;
        q.qy = (int)ry;
        q.qz = (int)rz;
      }
    }
  }
  return q;
}

// ---- A. candidates ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cand_count_kernel(const int *__restrict__ labels, const float *__restrict__ xyz,
                                                         int n, int nch, int *__restrict__ wcnt) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c = blockIdx.x, b = blockIdx.y;
  const int *L = labels + (size_t)b * n;
  const float *X = xyz + (size_t)b * 3 * n;
  const int p0 = c * CHUNK + w * SUB;
  int cnt = 0;
  for (int it = 0; it < SUB / 64; ++it) {
    const int base = p0 + it * 64;
    if (base >= n) break;  // uniform per wave
    cnt += __popcll(__ballot(load_pt(L, X, n, base + lane).cand));
  }
  if (lane == 0) wcnt[((size_t)b * nch + c) * WAVES + w] = cnt;
}

__global__ __launch_bounds__(256) void cand_scan_kernel(int E, int *__restrict__ wcnt, int *__restrict__ Mv) {
  __shared__ int part[256];
  const int tid = threadIdx.x, b = blockIdx.x;
  int *WC = wcnt + (size_t)b * E;
  const int per = (E + 255) / 256;
  const int lo = min(tid * per, E), hi = min(lo + per, E);
  int s = 0;
  for (int i = lo; i < hi; ++i) s += WC[i];
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int i = 0; i < 256; ++i) {
      const int t = part[i];
      part[i] = run;
      run += t;
    }
    Mv[b] = run;
  }
  __syncthreads();
  int run = part[tid];
  for (int i = lo; i < hi; ++i) {  // exclusive scan over (chunk, wave): the rank of the wave's first candidate
    const int t = WC[i];
    WC[i] = run;
    run += t;
  }
}

__global__ __launch_bounds__(256) void cand_scatter_kernel(const int *__restrict__ labels, const float *__restrict__ xyz,
                                                           int n, int nch, const int *__restrict__ wcnt,
                                                           int2 *__restrict__ cand) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c = blockIdx.x, b = blockIdx.y;
  const int *L = labels + (size_t)b * n;
  const float *X = xyz + (size_t)b * 3 * n;
  int2 *C = cand + (size_t)b * n;
  const int p0 = c * CHUNK + w * SUB;
  int run = wcnt[((size_t)b * nch + c) * WAVES + w];
  for (int it = 0; it < SUB / 64; ++it) {
    const int base = p0 + it * 64;
    if (base >= n) break;
    const Pt q = load_pt(L, X, n, base + lane);
    const unsigned long long m = __ballot(q.cand);
    if (q.cand)  // rank < M <= n: the count pass saw the same candidates
      C[run + lane_rank(m)] = make_int2((int)(((unsigned)q.qx & 0xffffu) | ((unsigned)q.qy << 16)), q.qz);
    run += __popcll(m);
  }
}

// ---- B. hypotheses --------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned mix32(unsigned x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

__global__ __launch_bounds__(256) void hyp_kernel(const int2 *__restrict__ cand, const int *__restrict__ Mv, int n,
                                                  int num_hyp, int tau_mm, unsigned seed, Hyp *__restrict__ hyp) {
  const int h = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (h >= num_hyp) return;
  const int M = Mv[b];
  Hyp o{0, 0, 0, 0, -1ll, 0ull};  // c0 = -1: no q passes the test
  if (M >= 3) {
    long long p[3][3];
    for (int k = 0; k < 3; ++k) {
      const unsigned r = mix32(seed ^ ((3u * (unsigned)h + (unsigned)k) * 0x9E3779B9u));
      const int i = (int)(((unsigned long long)r * (unsigned long long)M) >> 32);  // < M
      const int2 q = cand[(size_t)b * n + i];
      p[k][0] = (short)(q.x & 0xffff);
      p[k][1] = q.x >> 16;
      p[k][2] = q.y;
    }
    const long long ax = p[1][0] - p[0][0], ay = p[1][1] - p[0][1], az = p[1][2] - p[0][2];
    const long long bx = p[2][0] - p[0][0], by = p[2][1] - p[0][1], bz = p[2][2] - p[0][2];
    long long nv[3] = {ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx};
    const long long g = max(max(llabs(nv[0]), llabs(nv[1])), llabs(nv[2]));
    if (g > 0) {
      const int s = max(0, 64 - __clzll(g) - 30);
      for (int k = 0; k < 3; ++k) nv[k] = nv[k] < 0 ? -((-nv[k]) >> s) : nv[k] >> s;  // g keeps 30 bits: n' != 0
      const unsigned long long S = (unsigned long long)(nv[0] * nv[0] + nv[1] * nv[1] + nv[2] * nv[2]);  // < 2^62
      unsigned long long r = (unsigned long long)sqrt((double)S);
      while (r * r > S) --r;
      while ((r + 1) * (r + 1) <= S) ++r;
      const long long thr = (long long)tau_mm * (long long)r;
      o.nx = (int)nv[0];
      o.ny = (int)nv[1];
      o.nz = (int)nv[2];
      o.ok = 1;
      o.c0 = thr - (nv[0] * p[0][0] + nv[1] * p[0][1] + nv[2] * p[0][2]);
      o.thr2 = 2ull * (unsigned long long)thr;
    }
  }
  hyp[(size_t)b * num_hyp + h] = o;
}

// The hot loop.  A lane keeps TC candidates in registers; the hypothesis is the same for the whole wave, so its eight
// words come through the scalar cache and the inlier count is a ballot and a scalar add.
__global__ __launch_bounds__(256) void score_kernel(const int2 *__restrict__ cand, const int *__restrict__ Mv, int n,
                                                    int num_hyp, const Hyp *__restrict__ hyp,
                                                    unsigned *__restrict__ score) {
  __shared__ unsigned wsc[WAVES][MAX_HYP];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, b = blockIdx.y;
  const int M = Mv[b];
  const long long t0 = (long long)blockIdx.x * TILE;
  if (t0 >= M) return;  // uniform per block
  const int2 *C = cand + (size_t)b * n;
  int qx[TC], qy[TC], qz[TC];
  unsigned long long okm[TC];
#pragma unroll
  for (int j = 0; j < TC; ++j) {
    const long long i = t0 + j * 256 + tid;
    const bool ok = i < M;
    const int2 q = C[ok ? i : M - 1];  // slots past M read a real candidate and are masked out of the count
    qx[j] = (short)(q.x & 0xffff);
    qy[j] = q.x >> 16;
    qz[j] = q.y;
    okm[j] = __ballot(ok);
  }
  const Hyp *HT = hyp + (size_t)b * num_hyp;
  for (int h0 = 0; h0 < num_hyp; h0 += 4) {  // four hypotheses per scalar-load batch: one wait for the four of them
    Hyp hp[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) hp[u] = HT[min(h0 + u, num_hyp - 1)];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      unsigned c = 0;
#pragma unroll
      for (int j = 0; j < TC; ++j) c += (unsigned)__popcll(__ballot(inlier(hp[u], qx[j], qy[j], qz[j])) & okm[j]);
      if (lane == 0 && h0 + u < num_hyp) wsc[w][h0 + u] = c;
    }
  }
  __syncthreads();
  for (int h = tid; h < num_hyp; h += 256) {
    const unsigned s = (wsc[0][h] + wsc[1][h]) + (wsc[2][h] + wsc[3][h]);
    if (s) atomicAdd(&score[(size_t)b * num_hyp + h], s);
  }
}

// The winner of round r, with the stop rule (not found below min_inliers) and its removal band.
__global__ __launch_bounds__(256) void pselect_kernel(int num_hyp, int K, int r, int tau_mm, int rem_mm, int min_inliers,
                                                      const Hyp *__restrict__ hyp, const unsigned *__restrict__ score,
                                                      const int *__restrict__ Mv, PWin *__restrict__ win) {
  __shared__ unsigned long long best[256];
  const int tid = threadIdx.x, b = blockIdx.x;
  unsigned long long k = 0ull;
  for (int h = tid; h < num_hyp; h += 256) {
    const unsigned long long sc1 = hyp[(size_t)b * num_hyp + h].ok ? (unsigned long long)score[(size_t)b * num_hyp + h] + 1ull : 0ull;
    k = max(k, (sc1 << 10) | (unsigned long long)(1023 - h));
  }
  best[tid] = k;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) best[tid] = max(best[tid], best[tid + s]);
    __syncthreads();
  }
  if (tid == 0) {
    const unsigned long long top = best[0];
    const Hyp none{0, 0, 0, 0, -1ll, 0ull};
    PWin o;
    o.M = Mv[b];
    o.found = (top >> 10) != 0ull && (long long)((top >> 10) - 1ull) >= (long long)min_inliers;
    o.hyp = o.found ? 1023 - (int)(top & 1023ull) : 0;
    o.score = o.found ? (int)((top >> 10) - 1ull) : 0;
    o.h = o.found ? hyp[(size_t)b * num_hyp + o.hyp] : none;
    o.hr = o.h;
    if (o.found) {
      const long long L = (long long)(o.h.thr2 / (2ull * (unsigned long long)tau_mm));  // thr2 = 2 * tau * L exactly
      o.hr.c0 = o.h.c0 + (long long)(rem_mm - tau_mm) * L;                               // rem * L - n'.p0
      o.hr.thr2 = 2ull * (unsigned long long)rem_mm * (unsigned long long)L;
    }
    win[(size_t)b * K + r] = o;
  }
}

// ---- C. refinement ----------------------------------------------------------------------------------------------
// Block sum of N per-lane fp64 accumulators in the fixed order lane tree, waves 0..3; out[k] is written by thread k.
template <int N>
__device__ __forceinline__ void block_sum_store(double (&acc)[N], double (*ws)[N], double *__restrict__ out) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const double s = wave_sum_d(acc[k]);
    if (lane == 0) ws[w][k] = s;
  }
  __syncthreads();
  if (tid < N) out[tid] = ((ws[0][tid] + ws[1][tid]) + ws[2][tid]) + ws[3][tid];
}

// Refinement of plane r of frame b, batch entry by = b * K + r of a (chunk, frame * K) grid.  Which pixels are summed is
// the template parameter, everything else (per-lane, lane-tree, wave and chunk order) is written once, so plane 0 of
// uoc_support_planes has the bits of uoc_support_plane.
//   BY_INDEX false (K = 1, `map` = the labels): a candidate by load_pt that is an inlier of the winner's band;
//   BY_INDEX true  (`map` = the index map):     index[p] == r.
// A member has p < n: its coordinates are X[p], X[n + p], X[2 n + p].
template <bool BY_INDEX>
__device__ __forceinline__ bool member(const int *map, const float *X, int n, int p, int r, const PWin &wn) {
  if constexpr (BY_INDEX) {
    return p < n && map[p] == r;
  } else {
    const Pt q = load_pt(map, X, n, p);
    return q.cand && inlier(wn.h, q.qx, q.qy, q.qz);
  }
}

template <bool BY_INDEX>
__global__ __launch_bounds__(256) void plane_sum_kernel(const int *__restrict__ map, const float *__restrict__ xyz, int n,
                                                        int nch, int K, const PWin *__restrict__ win,
                                                        double *__restrict__ psum) {
  __shared__ double ws[WAVES][3];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c = blockIdx.x, by = blockIdx.y, b = by / K, r = by - b * K;
  const PWin wn = win[by];   // the <true> instantiation uses `found` only
  if (!wn.found) return;
  const int *MP = map + (size_t)b * n;
  const float *X = xyz + (size_t)b * 3 * n;
  const int p0 = c * CHUNK + w * SUB;
  double acc[3] = {0.0, 0.0, 0.0};
  for (int it = 0; it < SUB / 64; ++it) {
    const int base = p0 + it * 64;
    if (base >= n) break;
    const int p = base + lane;
    if (member<BY_INDEX>(MP, X, n, p, r, wn)) {
      acc[0] += (double)X[p];
      acc[1] += (double)X[(size_t)n + p];
      acc[2] += (double)X[2 * (size_t)n + p];
    }
  }
  block_sum_store<3>(acc, ws, psum + ((size_t)by * nch + c) * 3);
}

// Sum of column k of a [nch][N] table in chunk order.
template <int N>
__device__ __forceinline__ double chunk_sum(const double *__restrict__ t, int nch, int k) {
  double s = 0.0;
#pragma unroll 8
  for (int c = 0; c < nch; ++c) s += t[(size_t)c * N + k];
  return s;
}

template <bool BY_INDEX>
__global__ __launch_bounds__(256) void plane_mom_kernel(const int *__restrict__ map, const float *__restrict__ xyz, int n,
                                                        int nch, int K, const PWin *__restrict__ win,
                                                        const double *__restrict__ psum, double *__restrict__ pmom) {
  __shared__ double ws[WAVES][6];
  __shared__ double cs[3];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c = blockIdx.x, by = blockIdx.y, b = by / K, r = by - b * K;
  const PWin wn = win[by];   // the <true> instantiation uses `found` and `score` only
  if (!wn.found) return;
  if (tid < 3) cs[tid] = chunk_sum<3>(psum + (size_t)by * nch * 3, nch, tid) / wn.score;
  __syncthreads();
  const double c0 = cs[0], c1 = cs[1], c2 = cs[2];
  const int *MP = map + (size_t)b * n;
  const float *X = xyz + (size_t)b * 3 * n;
  const int p0 = c * CHUNK + w * SUB;
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int it = 0; it < SUB / 64; ++it) {
    const int base = p0 + it * 64;
    if (base >= n) break;
    const int p = base + lane;
    if (member<BY_INDEX>(MP, X, n, p, r, wn)) {
      const double dx = (double)X[p] - c0, dy = (double)X[(size_t)n + p] - c1, dz = (double)X[2 * (size_t)n + p] - c2;
      acc[0] += dx * dx;
      acc[1] += dx * dy;
      acc[2] += dx * dz;
      acc[3] += dy * dy;
      acc[4] += dy * dz;
      acc[5] += dz * dz;
    }
  }
  block_sum_store<6>(acc, ws, pmom + ((size_t)by * nch + c) * 6);
}

// The uoc_plane record and the fp64 frame F[NFR] of one plane from its centroid cs and centred moments ms (both already
// divided by the inlier count).  One thread.
__device__ __forceinline__ void fit_record(int found, int M, int score, int hyp, const double *cs, const double *ms,
                                           uoc_plane *__restrict__ out, double *__restrict__ F) {
  uoc_plane o;
  o.found = found;
  o.candidates = M;
  o.inliers = score;
  o.hyp = hyp;
  o.d = o.rms = 0.f;
  for (int k = 0; k < 3; ++k) o.normal[k] = o.centroid[k] = o.eig[k] = o.u[k] = o.v[k] = 0.f;
  for (int k = 0; k < NFR; ++k) F[k] = 0.0;
  if (found) {
    double a[3][3] = {{ms[0], ms[1], ms[2]}, {ms[1], ms[3], ms[4]}, {ms[2], ms[4], ms[5]}}, v[3][3];
    jacobi3(a, v);
    double lam[3], vec[3][3];
    sort_eig3(a, v, lam, vec);
    double nn[3] = {vec[2][0], vec[2][1], vec[2][2]};
    double d = -((nn[0] * cs[0] + nn[1] * cs[1]) + nn[2] * cs[2]);
    if (d < 0.0) {
      d = -d;
      for (int k = 0; k < 3; ++k) nn[k] = -nn[k];
    } else if (d == 0.0) {
      d = 0.0;
      sign_rule(nn);
    }
    double u[3], len = 0.0;
    for (int axis = 0; axis < 2; ++axis) {  // the camera x axis projected onto the plane, else the y axis
      for (int k = 0; k < 3; ++k) u[k] = (k == axis ? 1.0 : 0.0) - nn[axis] * nn[k];
      len = sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
      if (len >= 1e-6) break;
    }
    for (int k = 0; k < 3; ++k) u[k] /= len;
    const double vv[3] = {nn[1] * u[2] - nn[2] * u[1], nn[2] * u[0] - nn[0] * u[2], nn[0] * u[1] - nn[1] * u[0]};
    for (int k = 0; k < 3; ++k) {
      F[FR_N + k] = nn[k];
      F[FR_C + k] = cs[k];
      F[FR_U + k] = u[k];
      F[FR_V + k] = vv[k];
      o.normal[k] = (float)nn[k];
      o.centroid[k] = (float)cs[k];
      o.eig[k] = (float)fmax(lam[k], 0.0);  // as rms below: a rank-deficient covariance can leave -1e-20
      o.u[k] = (float)u[k];
      o.v[k] = (float)vv[k];
    }
    F[FR_D] = d;
    F[FR_FOUND] = 1.0;
    o.d = (float)d;
    o.rms = (float)sqrt(fmax(lam[2], 0.0));
  }
  *out = o;
}

__global__ __launch_bounds__(64) void pfit_kernel(int nch, const PWin *__restrict__ win, const double *__restrict__ psum,
                                                  const double *__restrict__ pmom, uoc_plane *__restrict__ planes,
                                                  double *__restrict__ frame) {
  __shared__ double cs[3], ms[6];
  const int tid = threadIdx.x, by = blockIdx.x;
  const int found = win[by].found, score = win[by].score;
  if (found) {
    if (tid < 3) cs[tid] = chunk_sum<3>(psum + (size_t)by * nch * 3, nch, tid) / score;
    if (tid >= 8 && tid < 14) ms[tid - 8] = chunk_sum<6>(pmom + (size_t)by * nch * 6, nch, tid - 8) / score;
  }
  __syncthreads();
  if (tid != 0) return;
  fit_record(found, win[by].M, score, win[by].hyp, cs, ms, planes + by, frame + (size_t)by * NFR);
}

// ---- D. objects against the plane ---------------------------------------------------------------------------------------
struct Frame {
  double n[3], d, c[3], u[3], v[3];
  bool found;
};
__device__ __forceinline__ Frame load_frame(const double *__restrict__ F) {
  Frame f;
  for (int k = 0; k < 3; ++k) {
    f.n[k] = F[FR_N + k];
    f.c[k] = F[FR_C + k];
    f.u[k] = F[FR_U + k];
    f.v[k] = F[FR_V + k];
  }
  f.d = F[FR_D];
  f.found = F[FR_FOUND] != 0.0;
  return f;
}
__device__ __forceinline__ double height_of(const Frame &f, const Pt &q) {
  return ((f.n[0] * (double)q.x + f.n[1] * (double)q.y) + f.n[2] * (double)q.z) + f.d;
}
__device__ __forceinline__ void inplane_of(const Frame &f, const Pt &q, double &a, double &bb) {
  const double dx = (double)q.x - f.c[0], dy = (double)q.y - f.c[1], dz = (double)q.z - f.c[2];
  a = (dx * f.u[0] + dy * f.u[1]) + dz * f.u[2];
  bb = (dx * f.v[0] + dy * f.v[1]) + dz * f.v[2];
}

__global__ __launch_bounds__(256) void obj_sum_kernel(const int *__restrict__ labels, const float *__restrict__ xyz,
                                                      int n, int nch, int per, const double *__restrict__ frame,
                                                      int *__restrict__ ocnt, unsigned long long *__restrict__ okey,
                                                      double *__restrict__ osum, float *__restrict__ height) {
  __shared__ int bcnt[NL];
  __shared__ unsigned long long bkey[NL][2];
  __shared__ double wsum[WAVES][NL][2];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c = blockIdx.x, b = blockIdx.y;
  const Frame f = load_frame(frame + (size_t)b * NFR);
  for (int i = tid; i < NL; i += 256) bcnt[i] = 0;
  for (int i = tid; i < NL * 2; i += 256) (&bkey[0][0])[i] = 0ull;
  for (int i = tid; i < WAVES * NL * 2; i += 256) (&wsum[0][0][0])[i] = 0.0;
  __syncthreads();
  const int *L = labels + (size_t)(b / per) * n;  // `per` batch entries (planes) share one image
  const float *X = xyz + (size_t)(b / per) * 3 * n;
  const int p0 = c * CHUNK + w * SUB;
  for (int it = 0; it < SUB / 64; ++it) {
    const int base = p0 + it * 64;
    if (base >= n) break;
    const int p = base + lane;
    const Pt q = load_pt(L, X, n, p);
    const double t = height_of(f, q);
    if (height && p < n) height[(size_t)b * n + p] = (f.found && q.point) ? (float)t : __int_as_float(0x7fc00000);
    if (!f.found) continue;  // uniform per frame
    double a, bb;
    inplane_of(f, q, a, bb);
    const bool valid = q.l >= 0 && q.point;
    unsigned long long rem = __ballot(valid);
    while (rem) {
      const int first = __ffsll((long long)rem) - 1;
      const int id = __builtin_amdgcn_readlane(q.l, first);
      const unsigned long long vm = __ballot(valid && q.l == id);
      rem &= ~vm;
      const bool gv = (vm >> lane) & 1ull;
      const double hi = wave_max_d(gv ? t : -INFINITY), lo = wave_max_d(gv ? -t : -INFINITY);
      const double sa = wave_sum_d(gv ? a : 0.0), sb = wave_sum_d(gv ? bb : 0.0);
      if (lane == 0) {
        atomicAdd(&bcnt[id], __popcll(vm));
        atomicMax(&bkey[id][0], dkey(hi));
        atomicMax(&bkey[id][1], dkey(lo));
        wsum[w][id][0] += sa;
        wsum[w][id][1] += sb;
      }
    }
  }
  if (!f.found) return;
  __syncthreads();
  for (int i = tid; i < NL; i += 256)
    if (bcnt[i]) atomicAdd(&ocnt[(size_t)b * NL + i], bcnt[i]);
  for (int i = tid; i < NL * 2; i += 256) {
    const unsigned long long v = (&bkey[0][0])[i];
    if (v) atomicMax(&okey[((size_t)b * NL + i / 2) * NKEY + (i & 1)], v);
  }
  for (int i = tid; i < NL * 2; i += 256) {
    const int l = i >> 1, k = i & 1;
    osum[((size_t)b * nch + c) * NL * 2 + i] = ((wsum[0][l][k] + wsum[1][l][k]) + wsum[2][l][k]) + wsum[3][l][k];
  }
}

__global__ __launch_bounds__(NL) void obj_mean_kernel(int nch, const double *__restrict__ frame,
                                                      const int *__restrict__ ocnt, const double *__restrict__ osum,
                                                      double *__restrict__ ofoot) {
  const int l = threadIdx.x, b = blockIdx.x;
  const int cnt = ocnt[(size_t)b * NL + l];
  double s0 = 0.0, s1 = 0.0;
  if (frame[(size_t)b * NFR + FR_FOUND] != 0.0 && cnt > 0) {
    const double *P = osum + ((size_t)b * nch * NL + l) * 2;
    s0 = chunk_sum<NL * 2>(P, nch, 0) / cnt;
    s1 = chunk_sum<NL * 2>(P, nch, 1) / cnt;
  }
  ofoot[((size_t)b * NL + l) * 2 + 0] = s0;
  ofoot[((size_t)b * NL + l) * 2 + 1] = s1;
}

__global__ __launch_bounds__(256) void obj_mom_kernel(const int *__restrict__ labels, const float *__restrict__ xyz,
                                                      int n, int nch, int per, const double *__restrict__ frame,
                                                      const double *__restrict__ ofoot, double *__restrict__ omom) {
  __shared__ double foot[NL][2];
  __shared__ double wmom[WAVES][NL][3];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c = blockIdx.x, b = blockIdx.y;
  const Frame f = load_frame(frame + (size_t)b * NFR);
  if (!f.found) return;
  for (int i = tid; i < NL * 2; i += 256) (&foot[0][0])[i] = ofoot[(size_t)b * NL * 2 + i];
  for (int i = tid; i < WAVES * NL * 3; i += 256) (&wmom[0][0][0])[i] = 0.0;
  __syncthreads();
  const int *L = labels + (size_t)(b / per) * n;  // `per` batch entries (planes) share one image
  const float *X = xyz + (size_t)(b / per) * 3 * n;
  const int p0 = c * CHUNK + w * SUB;
  for (int it = 0; it < SUB / 64; ++it) {
    const int base = p0 + it * 64;
    if (base >= n) break;
    const Pt q = load_pt(L, X, n, base + lane);
    double a, bb;
    inplane_of(f, q, a, bb);
    const bool valid = q.l >= 0 && q.point;
    unsigned long long rem = __ballot(valid);
    while (rem) {
      const int first = __ffsll((long long)rem) - 1;
      const int id = __builtin_amdgcn_readlane(q.l, first);
      const unsigned long long vm = __ballot(valid && q.l == id);
      rem &= ~vm;
      const bool gv = (vm >> lane) & 1ull;
      const double ra = gv ? a - foot[id][0] : 0.0, rb = gv ? bb - foot[id][1] : 0.0;
      const double m0 = wave_sum_d(ra * ra), m1 = wave_sum_d(ra * rb), m2 = wave_sum_d(rb * rb);
      if (lane == 0) {
        wmom[w][id][0] += m0;
        wmom[w][id][1] += m1;
        wmom[w][id][2] += m2;
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < NL * 3; i += 256) {
    const int l = i / 3, k = i - l * 3;
    omom[((size_t)b * nch + c) * NL * 3 + i] = ((wmom[0][l][k] + wmom[1][l][k]) + wmom[2][l][k]) + wmom[3][l][k];
  }
}

__global__ __launch_bounds__(NL) void obj_axis_kernel(int nch, const double *__restrict__ frame,
                                                      const int *__restrict__ ocnt,
                                                      const unsigned long long *__restrict__ okey,
                                                      const double *__restrict__ ofoot, const double *__restrict__ omom,
                                                      double *__restrict__ oaxis, uoc_plane_object *__restrict__ objs) {
  const int l = threadIdx.x, b = blockIdx.x;
  const int cnt = ocnt[(size_t)b * NL + l];
  uoc_plane_object o;
  o.count = 0;
  o.height_min = o.height_max = 0.f;
  o.foot[0] = o.foot[1] = o.axis[0] = o.axis[1] = 0.f;
  for (int k = 0; k < 3; ++k) o.cov2[k] = o.half[k] = o.center[k] = 0.f;
  double e0 = 0.0, e1 = 0.0;
  if (frame[(size_t)b * NFR + FR_FOUND] != 0.0 && cnt > 0 && l > 0) {
    const double *P = omom + ((size_t)b * nch * NL + l) * 3;
    const double caa = chunk_sum<NL * 3>(P, nch, 0) / cnt, cab = chunk_sum<NL * 3>(P, nch, 1) / cnt,
                 cbb = chunk_sum<NL * 3>(P, nch, 2) / cnt;
    // major axis of [[caa, cab], [cab, cbb]]: eigenvalues m +- s, vector (s + hd, cab) or (cab, s - hd), the one
    // without cancellation
    const double hd = 0.5 * (caa - cbb), s = sqrt(hd * hd + cab * cab);
    e0 = 1.0;
    e1 = 0.0;
    if (s > 0.0) {
      const double x = hd >= 0.0 ? s + hd : cab, y = hd >= 0.0 ? cab : s - hd;
      const double len = sqrt(x * x + y * y);
      e0 = x / len;
      e1 = y / len;
      if ((fabs(e1) > fabs(e0) ? e1 : e0) < 0.0) {
        e0 = -e0;
        e1 = -e1;
      }
    }
    const unsigned long long *K = okey + ((size_t)b * NL + l) * NKEY;
    o.count = cnt;
    o.height_max = (float)ddecode(K[K_TMAX]);
    o.height_min = (float)(-ddecode(K[K_TMIN]));
    o.foot[0] = (float)ofoot[((size_t)b * NL + l) * 2 + 0];
    o.foot[1] = (float)ofoot[((size_t)b * NL + l) * 2 + 1];
    o.cov2[0] = (float)caa;
    o.cov2[1] = (float)cab;
    o.cov2[2] = (float)cbb;
    o.axis[0] = (float)e0;
    o.axis[1] = (float)e1;
  }
  oaxis[((size_t)b * NL + l) * 2 + 0] = e0;
  oaxis[((size_t)b * NL + l) * 2 + 1] = e1;
  objs[(size_t)b * NL + l] = o;
}

__global__ __launch_bounds__(256) void obj_extent_kernel(const int *__restrict__ labels, const float *__restrict__ xyz,
                                                         int n, int per, const double *__restrict__ frame,
                                                         const double *__restrict__ ofoot,
                                                         const double *__restrict__ oaxis,
                                                         unsigned long long *__restrict__ okey) {
  __shared__ double foot[NL][2], ax[NL][2];
  __shared__ unsigned long long bext[NL][4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c = blockIdx.x, b = blockIdx.y;
  const Frame f = load_frame(frame + (size_t)b * NFR);
  if (!f.found) return;
  for (int i = tid; i < NL * 2; i += 256) {
    (&foot[0][0])[i] = ofoot[(size_t)b * NL * 2 + i];
    (&ax[0][0])[i] = oaxis[(size_t)b * NL * 2 + i];
  }
  for (int i = tid; i < NL * 4; i += 256) (&bext[0][0])[i] = 0ull;
  __syncthreads();
  const int *L = labels + (size_t)(b / per) * n;  // `per` batch entries (planes) share one image
  const float *X = xyz + (size_t)(b / per) * 3 * n;
  const int p0 = c * CHUNK + w * SUB;
  for (int it = 0; it < SUB / 64; ++it) {
    const int base = p0 + it * 64;
    if (base >= n) break;
    const Pt q = load_pt(L, X, n, base + lane);
    double a, bb;
    inplane_of(f, q, a, bb);
    const bool valid = q.l >= 0 && q.point;
    unsigned long long rem = __ballot(valid);
    while (rem) {
      const int first = __ffsll((long long)rem) - 1;
      const int id = __builtin_amdgcn_readlane(q.l, first);
      const unsigned long long vm = __ballot(valid && q.l == id);
      rem &= ~vm;
      const bool gv = (vm >> lane) & 1ull;
      const double ra = a - foot[id][0], rb = bb - foot[id][1];
      const double d0 = ra * ax[id][0] + rb * ax[id][1], d1 = rb * ax[id][0] - ra * ax[id][1];
      const double h0 = wave_max_d(gv ? d0 : -INFINITY), l0 = wave_max_d(gv ? -d0 : -INFINITY);
      const double h1 = wave_max_d(gv ? d1 : -INFINITY), l1 = wave_max_d(gv ? -d1 : -INFINITY);
      if (lane == 0) {
        atomicMax(&bext[id][0], dkey(h0));
        atomicMax(&bext[id][1], dkey(l0));
        atomicMax(&bext[id][2], dkey(h1));
        atomicMax(&bext[id][3], dkey(l1));
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < NL * 4; i += 256) {
    const unsigned long long v = (&bext[0][0])[i];
    if (v) atomicMax(&okey[((size_t)b * NL + i / 4) * NKEY + K_E0 + (i & 3)], v);
  }
}

__global__ __launch_bounds__(NL) void obj_box_kernel(const double *__restrict__ frame, const double *__restrict__ ofoot,
                                                     const double *__restrict__ oaxis,
                                                     const unsigned long long *__restrict__ okey,
                                                     uoc_plane_object *__restrict__ objs) {
  const int l = threadIdx.x, b = blockIdx.x;
  uoc_plane_object *o = objs + (size_t)b * NL + l;
  if (o->count <= 0) return;
  const Frame f = load_frame(frame + (size_t)b * NFR);
  const unsigned long long *K = okey + ((size_t)b * NL + l) * NKEY;
  const double hi[3] = {ddecode(K[K_E0 + 0]), ddecode(K[K_E0 + 2]), ddecode(K[K_TMAX])};
  const double lo[3] = {-ddecode(K[K_E0 + 1]), -ddecode(K[K_E0 + 3]), -ddecode(K[K_TMIN])};
  double mid[3];
  for (int k = 0; k < 3; ++k) {
    mid[k] = 0.5 * (lo[k] + hi[k]);
    o->half[k] = (float)(0.5 * (hi[k] - lo[k]));
  }
  const double e0 = oaxis[((size_t)b * NL + l) * 2 + 0], e1 = oaxis[((size_t)b * NL + l) * 2 + 1];
  const double a = ofoot[((size_t)b * NL + l) * 2 + 0] + (mid[0] * e0 - mid[1] * e1);
  const double bb = ofoot[((size_t)b * NL + l) * 2 + 1] + (mid[0] * e1 + mid[1] * e0);
  for (int i = 0; i < 3; ++i) o->center[i] = (float)(f.c[i] + ((a * f.u[i] + bb * f.v[i]) + mid[2] * f.n[i]));
}

// ==== several planes (uoc_support_planes) ===========================================================
// Sequential extraction: rounds of hyp / score / select on a candidate list that shrinks by the winner's removal band.
// M_r and the stop flag live on the device: a stopped frame has M = 0 from then on, so hyp_kernel writes degenerate
// hypotheses, score_kernel's blocks exit at once and the round's winner is "not found".
constexpr int MAX_PLANES = UOC_PLANES_MAX;
constexpr int FRINGE = 16;  // index map: FRINGE + r marks the removal band of plane r outside its inliers

__device__ __forceinline__ void unpack_q(const int2 q, int &qx, int &qy, int &qz) {
  qx = (short)(q.x & 0xffff);
  qy = q.x >> 16;
  qz = q.y;
}

// Re-compaction of the survivors, pass 1: survivors per wave; a wave owns SUB consecutive list entries.
__global__ __launch_bounds__(256) void recount_kernel(const int2 *__restrict__ src, const int *__restrict__ Mv, int n,
                                                      int nch, int K, int r, const PWin *__restrict__ win,
                                                      int *__restrict__ wcnt) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c = blockIdx.x, b = blockIdx.y;
  const PWin *wn = win + (size_t)b * K + r;
  if (!wn->found) return;  // a stopped frame: uniform per block
  const Hyp hr = wn->hr;
  const int M = Mv[b];
  const int2 *S = src + (size_t)b * n;
  const long long i0 = (long long)c * CHUNK + (long long)w * SUB;
  int cnt = 0;
  for (int it = 0; it < SUB / 64; ++it) {
    const long long base = i0 + it * 64;
    if (base >= M) break;  // uniform per wave
    const long long i = base + lane;
    bool keep = false;
    if (i < M) {
      int qx, qy, qz;
      unpack_q(S[i], qx, qy, qz);
      keep = !inlier(hr, qx, qy, qz);
    }
    cnt += __popcll(__ballot(keep));
  }
  if (lane == 0) wcnt[((size_t)b * nch + c) * WAVES + w] = cnt;
}

// Pass 2: every block sums the wave counts in front of it (integers: any order), then scatters its survivors at their
// raster-order rank; the last block also writes M_{r+1}.  A stopped frame gets M_{r+1} = 0 and nothing else.
__global__ __launch_bounds__(256) void rescatter_kernel(const int2 *__restrict__ src, int2 *__restrict__ dst,
                                                        const int *__restrict__ Mv, int *__restrict__ Mnext, int n,
                                                        int nch, int K, int r, const PWin *__restrict__ win,
                                                        const int *__restrict__ wcnt) {
  __shared__ int part[256];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c = blockIdx.x, b = blockIdx.y;
  const PWin *wn = win + (size_t)b * K + r;
  if (!wn->found) {
    if (c == nch - 1 && tid == 0) Mnext[b] = 0;
    return;
  }
  const Hyp hr = wn->hr;
  const int M = Mv[b];
  const int *WC = wcnt + (size_t)b * nch * WAVES;
  int s = 0;
  for (int i = tid; i < c * WAVES; i += 256) s += WC[i];
  part[tid] = s;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) part[tid] += part[tid + st];
    __syncthreads();
  }
  int run = part[0];
  for (int k = 0; k < w; ++k) run += WC[c * WAVES + k];
  if (c == nch - 1 && tid == 0) Mnext[b] = part[0] + ((WC[c * WAVES] + WC[c * WAVES + 1]) + (WC[c * WAVES + 2] + WC[c * WAVES + 3]));
  const int2 *S = src + (size_t)b * n;
  int2 *D = dst + (size_t)b * n;
  const long long i0 = (long long)c * CHUNK + (long long)w * SUB;
  for (int it = 0; it < SUB / 64; ++it) {
    const long long base = i0 + it * 64;
    if (base >= M) break;
    const long long i = base + lane;
    bool keep = false;
    int2 q = make_int2(0, 0);
    if (i < M) {
      q = S[i];
      int qx, qy, qz;
      unpack_q(q, qx, qy, qz);
      keep = !inlier(hr, qx, qy, qz);
    }
    const unsigned long long m = __ballot(keep);
    if (keep) D[run + lane_rank(m)] = q;  // rank < M_{r+1} <= M_r <= n: pass 1 counted the same survivors
    run += __popcll(m);
  }
}

// The index map: every pixel tests the winners in order, the first whose removal band holds it claims it.
__global__ __launch_bounds__(256) void index_kernel(const int *__restrict__ labels, const float *__restrict__ xyz, int n,
                                                    int K, const PWin *__restrict__ win, int *__restrict__ index,
                                                    int *__restrict__ pcnt) {
  __shared__ int bcnt[MAX_PLANES];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c = blockIdx.x, b = blockIdx.y;
  if (tid < MAX_PLANES) bcnt[tid] = 0;
  __syncthreads();
  const int *L = labels + (size_t)b * n;
  const float *X = xyz + (size_t)b * 3 * n;
  const PWin *WN = win + (size_t)b * K;
  int *IX = index + (size_t)b * n;
  const int p0 = c * CHUNK + w * SUB;
  int cnt[MAX_PLANES];
#pragma unroll
  for (int r = 0; r < MAX_PLANES; ++r) cnt[r] = 0;
  for (int it = 0; it < SUB / 64; ++it) {
    const int base = p0 + it * 64;
    if (base >= n) break;
    const int p = base + lane;
    const Pt q = load_pt(L, X, n, p);
    int idx = q.cand ? -1 : -2;
#pragma unroll
    for (int r = 0; r < MAX_PLANES; ++r) {
      if (r < K && WN[r].found) {  // uniform: found planes are the slots 0..count-1
        const bool claim = q.cand && idx == -1 && inlier(WN[r].hr, q.qx, q.qy, q.qz);
        if (claim) idx = inlier(WN[r].h, q.qx, q.qy, q.qz) ? r : FRINGE + r;
        cnt[r] += __popcll(__ballot(claim));
      }
    }
    if (p < n) IX[p] = idx;
  }
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < MAX_PLANES; ++r)
      if (cnt[r]) atomicAdd(&bcnt[r], cnt[r]);
  }
  __syncthreads();
  if (tid < K && bcnt[tid]) atomicAdd(&pcnt[(size_t)b * K + tid], bcnt[tid]);
}

// In-plane extents of every plane's inliers through the ordered keys: max a, max -a, max b, max -b.
__global__ __launch_bounds__(256) void pextent_kernel(const float *__restrict__ xyz, const int *__restrict__ index, int n,
                                                      int K, const double *__restrict__ frame,
                                                      unsigned long long *__restrict__ pext) {
  __shared__ double fr[MAX_PLANES][NFR];
  __shared__ unsigned long long bext[MAX_PLANES][4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c = blockIdx.x, b = blockIdx.y;
  if (frame[(size_t)b * K * NFR + FR_FOUND] == 0.0) return;  // no plane 0: no plane at all
  for (int i = tid; i < K * NFR; i += 256) (&fr[0][0])[i] = frame[(size_t)b * K * NFR + i];
  for (int i = tid; i < MAX_PLANES * 4; i += 256) (&bext[0][0])[i] = 0ull;
  __syncthreads();
  const float *X = xyz + (size_t)b * 3 * n;
  const int *IX = index + (size_t)b * n;
  const int p0 = c * CHUNK + w * SUB;
  for (int it = 0; it < SUB / 64; ++it) {
    const int base = p0 + it * 64;
    if (base >= n) break;
    const int p = base + lane;
    const int idx = p < n ? IX[p] : -2;
    const bool valid = idx >= 0 && idx < K;
    double x = 0.0, y = 0.0, z = 0.0;
    if (valid) {
      x = (double)X[p];
      y = (double)X[(size_t)n + p];
      z = (double)X[2 * (size_t)n + p];
    }
    unsigned long long rem = __ballot(valid);
    while (rem) {
      const int first = __ffsll((long long)rem) - 1;
      const int r = __builtin_amdgcn_readlane(idx, first);
      const unsigned long long vm = __ballot(valid && idx == r);
      rem &= ~vm;
      const bool gv = (vm >> lane) & 1ull;
      const double *F = fr[r];
      const double dx = x - F[FR_C + 0], dy = y - F[FR_C + 1], dz = z - F[FR_C + 2];
      const double a = (dx * F[FR_U + 0] + dy * F[FR_U + 1]) + dz * F[FR_U + 2];
      const double bb = (dx * F[FR_V + 0] + dy * F[FR_V + 1]) + dz * F[FR_V + 2];
      const double ha = wave_max_d(gv ? a : -INFINITY), la = wave_max_d(gv ? -a : -INFINITY);
      const double hb = wave_max_d(gv ? bb : -INFINITY), lb = wave_max_d(gv ? -bb : -INFINITY);
      if (lane == 0) {
        atomicMax(&bext[r][0], dkey(ha));
        atomicMax(&bext[r][1], dkey(la));
        atomicMax(&bext[r][2], dkey(hb));
        atomicMax(&bext[r][3], dkey(lb));
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < K * 4; i += 256) {
    const unsigned long long v = (&bext[0][0])[i];
    if (v) atomicMax(&pext[(size_t)b * K * 4 + i], v);
  }
}

__global__ __launch_bounds__(64) void pinfo_kernel(int K, const PWin *__restrict__ win, const double *__restrict__ frame,
                                                   const int *__restrict__ pcnt,
                                                   const unsigned long long *__restrict__ pext,
                                                   uoc_plane_info *__restrict__ info, int *__restrict__ count) {
  const int r = threadIdx.x, b = blockIdx.x;
  if (r == 0) {
    int cnt = 0;
    for (int k = 0; k < K; ++k) cnt += win[(size_t)b * K + k].found;
    count[b] = cnt;
  }
  if (r >= K) return;
  const size_t by = (size_t)b * K + r;
  uoc_plane_info o;
  o.round_candidates = win[by].M;
  o.removed = 0;
  o.cos0 = o.offset0 = 0.f;
  for (int k = 0; k < 4; ++k) o.extent[k] = 0.f;
  if (win[by].found) {
    const double *F0 = frame + (size_t)b * K * NFR, *F = frame + by * NFR;
    o.removed = pcnt[by];
    o.cos0 = (float)((F[FR_N + 0] * F0[FR_N + 0] + F[FR_N + 1] * F0[FR_N + 1]) + F[FR_N + 2] * F0[FR_N + 2]);
    o.offset0 = (float)(((F0[FR_N + 0] * F[FR_C + 0] + F0[FR_N + 1] * F[FR_C + 1]) + F0[FR_N + 2] * F[FR_C + 2]) + F0[FR_D]);
    const unsigned long long *E = pext + by * 4;
    o.extent[0] = (float)(-ddecode(E[1]));
    o.extent[1] = (float)ddecode(E[0]);
    o.extent[2] = (float)(-ddecode(E[3]));
    o.extent[3] = (float)ddecode(E[2]);
  }
  info[by] = o;
}

// Workspace layout of both entry points (uoc_plane_workspace_bytes is K = 1).  The zeroed part comes first.
struct PWs {
  unsigned *score;            // [K][B][num_hyp]         zeroed
  int *ocnt;                  // [B*K][NL]               zeroed
  unsigned long long *okey;   // [B*K][NL][NKEY]         zeroed
  int *pcnt;                  // [B*K]                   zeroed
  unsigned long long *pext;   // [B*K][4]                zeroed
  int *wcnt;                  // [B][nch][WAVES]  candidates per wave, then rank bases
  int *M;                     // [K+1][B]; [B] if K = 1
  int2 *cand[2];              // [B][n] each, x | y << 16, z: ping-pong; the second only if K > 1
  Hyp *hyp;                   // [B][num_hyp]
  PWin *win;                  // [B*K]
  double *psum;               // [B*K][nch][3]
  double *pmom;               // [B*K][nch][6]
  double *frame;              // [B*K][NFR]
  double *osum;               // [B*K][nch][NL][2]
  double *omom;               // [B*K][nch][NL][3]
  double *ofoot;              // [B*K][NL][2]
  double *oaxis;              // [B*K][NL][2]
  size_t zero_bytes, total;
};
PWs pcarve(void *base, int B, size_t n, int nch, int num_hyp, int K) {
  PWs w;
  Carver cv(base);
  const size_t BK = (size_t)B * K;
  w.score = cv.take<unsigned>(BK * num_hyp);
  w.ocnt = cv.take<int>(BK * NL);
  w.okey = cv.take<unsigned long long>(BK * NL * NKEY);
  w.pcnt = cv.take<int>(BK);
  w.pext = cv.take<unsigned long long>(BK * 4);
  w.zero_bytes = cv.total();
  w.wcnt = cv.take<int>((size_t)B * nch * WAVES);
  w.M = cv.take<int>((size_t)(K > 1 ? K + 1 : 1) * B);
  w.cand[0] = cv.take<int2>((size_t)B * n);
  w.cand[1] = K > 1 ? cv.take<int2>((size_t)B * n) : nullptr;
  w.hyp = cv.take<Hyp>((size_t)B * num_hyp);
  w.win = cv.take<PWin>(BK);
  w.psum = cv.take<double>(BK * nch * 3);
  w.pmom = cv.take<double>(BK * nch * 6);
  w.frame = cv.take<double>(BK * NFR);
  w.osum = cv.take<double>(BK * nch * NL * 2);
  w.omom = cv.take<double>(BK * nch * NL * 3);
  w.ofoot = cv.take<double>(BK * NL * 2);
  w.oaxis = cv.take<double>(BK * NL * 2);
  w.total = cv.total();
  return w;
}

// ---- host side: what the two entry points share; `who` is the entry point's name in the messages ----------------
int check_shape(const char *who, int B, int max_B, int H, int W) {
  UOC_REQUIRE(B > 0 && B <= max_B && H > 0 && W > 0, "%s: bad shape B=%d H=%d W=%d", who, B, H, W);
  UOC_REQUIRE((long long)B * H * W <= INT_MAX, "%s: B*H*W = %lld exceeds int32 indexing", who, (long long)B * H * W);
  return UOC_OK;
}
int check_hyp(const char *who, int num_hyp, int tau_mm) {
  UOC_REQUIRE(num_hyp >= 1 && num_hyp <= MAX_HYP, "%s: num_hyp = %d outside [1, %d]", who, num_hyp, MAX_HYP);
  UOC_REQUIRE(tau_mm >= 1 && tau_mm <= 1000, "%s: tau_mm = %d outside [1, 1000]", who, tau_mm);
  return UOC_OK;
}

// Zero the workspace's head and compact the candidates into w.cand[0], their count into w.M[0..B).
int launch_candidates(int kc, const int *d_labels, const float *d_xyz, int B, int n, int nch, void *d_ws, const PWs &w,
                      hipStream_t st) {
  const dim3 grid(nch, B), blk(256);
  ProfScope prof(kc, st, 0.0, (double)B * n * (2 * 16.0 + 8.0));
  UOC_HIP_CHECK(hipMemsetAsync(d_ws, 0, w.zero_bytes, st));
  hipLaunchKernelGGL(cand_count_kernel, grid, blk, 0, st, d_labels, d_xyz, n, nch, w.wcnt);
  hipLaunchKernelGGL(cand_scan_kernel, dim3(B), blk, 0, st, nch * WAVES, w.wcnt, w.M);
  hipLaunchKernelGGL(cand_scatter_kernel, grid, blk, 0, st, d_labels, d_xyz, n, nch, w.wcnt, w.cand[0]);
  return UOC_OK;
}

// The objects of every frame against each of its K planes; the height map (K = 1 only) may be null.
void launch_objects(int kc, const int *d_labels, const float *d_xyz, int B, int n, int nch, int K, const PWs &w,
                    uoc_plane_object *d_objs, float *d_height, hipStream_t st) {
  const dim3 gridk(nch, B * K), blk(256);
  ProfScope prof(kc, st, 0.0, (double)B * n * (3 * 16.0 * K + (d_height ? 4.0 : 0.0)));
  hipLaunchKernelGGL(obj_sum_kernel, gridk, blk, 0, st, d_labels, d_xyz, n, nch, K, w.frame, w.ocnt, w.okey, w.osum, d_height);
  hipLaunchKernelGGL(obj_mean_kernel, dim3(B * K), dim3(NL), 0, st, nch, w.frame, w.ocnt, w.osum, w.ofoot);
  hipLaunchKernelGGL(obj_mom_kernel, gridk, blk, 0, st, d_labels, d_xyz, n, nch, K, w.frame, w.ofoot, w.omom);
  hipLaunchKernelGGL(obj_axis_kernel, dim3(B * K), dim3(NL), 0, st, nch, w.frame, w.ocnt, w.okey, w.ofoot, w.omom, w.oaxis, d_objs);
  hipLaunchKernelGGL(obj_extent_kernel, gridk, blk, 0, st, d_labels, d_xyz, n, K, w.frame, w.ofoot, w.oaxis, w.okey);
  hipLaunchKernelGGL(obj_box_kernel, dim3(B * K), dim3(NL), 0, st, w.frame, w.ofoot, w.oaxis, w.okey, d_objs);
}

}  // namespace
}  // namespace uoc

using namespace uoc;

extern "C" {

size_t uoc_plane_workspace_bytes(int B, int H, int W, int num_hyp) {
  if (B <= 0 || B > 65535 || H <= 0 || W <= 0 || (long long)B * H * W > INT_MAX || num_hyp < 1 || num_hyp > MAX_HYP) return 0;
  const long long n = (long long)H * W;
  return pcarve(nullptr, B, (size_t)n, (int)((n + CHUNK - 1) / CHUNK), num_hyp, 1).total;
}

int uoc_support_plane(const int32_t *d_labels, const float *d_xyz, int B, int H, int W, int num_hyp, int tau_mm,
                      uint32_t seed, uoc_plane *d_planes, uoc_plane_object *d_objs, float *d_height, void *d_ws,
                      size_t ws_bytes, void *stream) {
  UOC_REQUIRE(d_labels && d_xyz && d_planes && d_objs && d_ws, "uoc_support_plane: null labels / xyz / planes / objects / workspace");
  if (int rc = check_shape("uoc_support_plane", B, 65535, H, W)) return rc;
  if (int rc = check_hyp("uoc_support_plane", num_hyp, tau_mm)) return rc;
  const int n = H * W;
  const int nch = (int)(((long long)n + CHUNK - 1) / CHUNK);
  const PWs w = pcarve(d_ws, B, (size_t)n, nch, num_hyp, 1);
  UOC_REQUIRE(ws_bytes >= w.total, "uoc_support_plane: workspace %zu < %zu bytes", ws_bytes, w.total);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(nch, B), blk(256);
  const double px = (double)B * n;
  if (int rc = launch_candidates(KC_PLANE_CAND, d_labels, d_xyz, B, n, nch, d_ws, w, st)) return rc;
  {
    ProfScope prof(KC_PLANE_HYP, st, 0.0, (double)B * num_hyp * (24.0 + sizeof(Hyp)));
    hipLaunchKernelGGL(hyp_kernel, dim3((num_hyp + 255) / 256, B), blk, 0, st, w.cand[0], w.M, n, num_hyp, tau_mm, seed, w.hyp);
  }
  {
    ProfScope prof(KC_PLANE_SCORE, st, 0.0, px * 8.0);
    hipLaunchKernelGGL(score_kernel, dim3((n + TILE - 1) / TILE, B), blk, 0, st, w.cand[0], w.M, n, num_hyp, w.hyp, w.score);
    // one round, no stop rule, removal band = inlier band
    hipLaunchKernelGGL(pselect_kernel, dim3(B), blk, 0, st, num_hyp, 1, 0, tau_mm, tau_mm, 0, w.hyp, w.score, w.M, w.win);
  }
  {
    ProfScope prof(KC_PLANE_REFINE, st, 0.0, px * 2 * 16.0);
    hipLaunchKernelGGL(plane_sum_kernel<false>, grid, blk, 0, st, d_labels, d_xyz, n, nch, 1, w.win, w.psum);
    hipLaunchKernelGGL(plane_mom_kernel<false>, grid, blk, 0, st, d_labels, d_xyz, n, nch, 1, w.win, w.psum, w.pmom);
    hipLaunchKernelGGL(pfit_kernel, dim3(B), dim3(64), 0, st, nch, w.win, w.psum, w.pmom, d_planes, w.frame);
  }
  launch_objects(KC_PLANE_OBJECTS, d_labels, d_xyz, B, n, nch, 1, w, d_objs, d_height, st);
  UOC_LAUNCH_CHECK();
  return UOC_OK;
}

size_t uoc_planes_workspace_bytes(int B, int H, int W, int num_hyp, int max_planes) {
  if (B <= 0 || H <= 0 || W <= 0 || (long long)B * H * W > INT_MAX || num_hyp < 1 || num_hyp > MAX_HYP ||
      max_planes < 1 || max_planes > MAX_PLANES || (long long)B * max_planes > 65535)
    return 0;
  const long long n = (long long)H * W;
  return pcarve(nullptr, B, (size_t)n, (int)((n + CHUNK - 1) / CHUNK), num_hyp, max_planes).total;
}

int uoc_support_planes(const int32_t *d_labels, const float *d_xyz, int B, int H, int W, int max_planes, int num_hyp,
                       int tau_mm, int rem_mm, int min_inliers, uint32_t seed, int32_t *d_count, uoc_plane *d_planes,
                       uoc_plane_info *d_info, int32_t *d_index, uoc_plane_object *d_objs, void *d_ws, size_t ws_bytes,
                       void *stream) {
  UOC_REQUIRE(d_labels && d_xyz && d_count && d_planes && d_info && d_index && d_ws,
              "uoc_support_planes: null labels / xyz / count / planes / info / index / workspace");
  if (int rc = check_shape("uoc_support_planes", B, INT_MAX, H, W)) return rc;
  UOC_REQUIRE(max_planes >= 1 && max_planes <= MAX_PLANES, "uoc_support_planes: max_planes = %d outside [1, %d]", max_planes, MAX_PLANES);
  UOC_REQUIRE((long long)B * max_planes <= 65535, "uoc_support_planes: B * max_planes = %lld above 65535", (long long)B * max_planes);
  if (int rc = check_hyp("uoc_support_planes", num_hyp, tau_mm)) return rc;
  UOC_REQUIRE(rem_mm >= tau_mm && rem_mm <= 1000, "uoc_support_planes: rem_mm = %d outside [tau_mm = %d, 1000]", rem_mm, tau_mm);
  UOC_REQUIRE(min_inliers >= 3, "uoc_support_planes: min_inliers = %d below 3", min_inliers);
  const int K = max_planes, n = H * W;
  const int nch = (int)(((long long)n + CHUNK - 1) / CHUNK);
  const PWs w = pcarve(d_ws, B, (size_t)n, nch, num_hyp, K);
  UOC_REQUIRE(ws_bytes >= w.total, "uoc_support_planes: workspace %zu < %zu bytes", ws_bytes, w.total);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(nch, B), gridk(nch, B * K), blk(256);
  const double px = (double)B * n;
  if (int rc = launch_candidates(KC_PLANES_CAND, d_labels, d_xyz, B, n, nch, d_ws, w, st)) return rc;
  {
    ProfScope prof(KC_PLANES_ROUNDS, st, 0.0, px * 8.0 * K);
    for (int r = 0; r < K; ++r) {
      const int2 *src = w.cand[r & 1];
      const int *Mr = w.M + (size_t)r * B;
      unsigned *score = w.score + (size_t)r * B * num_hyp;
      hipLaunchKernelGGL(hyp_kernel, dim3((num_hyp + 255) / 256, B), blk, 0, st, src, Mr, n, num_hyp, tau_mm, seed + (uint32_t)r, w.hyp);
      hipLaunchKernelGGL(score_kernel, dim3((n + TILE - 1) / TILE, B), blk, 0, st, src, Mr, n, num_hyp, w.hyp, score);
      hipLaunchKernelGGL(pselect_kernel, dim3(B), blk, 0, st, num_hyp, K, r, tau_mm, rem_mm, min_inliers, w.hyp, score, Mr, w.win);
      if (r + 1 < K) {
        hipLaunchKernelGGL(recount_kernel, grid, blk, 0, st, src, Mr, n, nch, K, r, w.win, w.wcnt);
        hipLaunchKernelGGL(rescatter_kernel, grid, blk, 0, st, src, w.cand[(r + 1) & 1], Mr, w.M + (size_t)(r + 1) * B, n, nch, K, r, w.win, w.wcnt);
      }
    }
  }
  {
    ProfScope prof(KC_PLANES_INDEX, st, 0.0, px * 20.0);
    hipLaunchKernelGGL(index_kernel, grid, blk, 0, st, d_labels, d_xyz, n, K, w.win, d_index, w.pcnt);
  }
  {
    ProfScope prof(KC_PLANES_REFINE, st, 0.0, px * 16.0 * (2 * K + 1));
    hipLaunchKernelGGL(plane_sum_kernel<true>, gridk, blk, 0, st, d_index, d_xyz, n, nch, K, w.win, w.psum);
    hipLaunchKernelGGL(plane_mom_kernel<true>, gridk, blk, 0, st, d_index, d_xyz, n, nch, K, w.win, w.psum, w.pmom);
    hipLaunchKernelGGL(pfit_kernel, dim3(B * K), dim3(64), 0, st, nch, w.win, w.psum, w.pmom, d_planes, w.frame);
    hipLaunchKernelGGL(pextent_kernel, grid, blk, 0, st, d_xyz, d_index, n, K, w.frame, w.pext);
    hipLaunchKernelGGL(pinfo_kernel, dim3(B), dim3(64), 0, st, K, w.win, w.frame, w.pcnt, w.pext, d_info, d_count);
  }
  if (d_objs) launch_objects(KC_PLANES_OBJECTS, d_labels, d_xyz, B, n, nch, K, w, d_objs, nullptr, st);
  UOC_LAUNCH_CHECK();
  return UOC_OK;
}
}
