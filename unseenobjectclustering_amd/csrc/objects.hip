// Per-object point clouds and 3D statistics from label maps (include/uoc_hip.h, uoc_objects).
//
// Input per frame b: labels [H][W] int32 (object ids 1..127, anything else is background) and the XYZ planes
// [3][H][W] fp32 metres; optionally C <= 8 attribute planes [C][H][W].  A valid point is an object pixel whose
// x, y, z are finite with z > 0.
//
// Launches (grid (chunk, frame) for the pixel passes, one block of 128 label threads per frame otherwise):
//   memset        zero the integer statistics and the extent keys
//   count_kernel  per chunk: pixels / box / AABB (order-free integer atomics), per-wave valid counts, fp64 sums of x, y, z
//   reduce_kernel per (frame, label): chunk sums in chunk order -> centroid; per-wave rank bases; kept counts and their
//                 exclusive scan over the labels of the frame
//   scatter_kernel per chunk: raster-order rank of every valid point -> packed points / attributes / pixel indices;
//                 fp64 centred second moments per chunk
//   moments_kernel per (frame, label): moments in chunk order -> covariance, cyclic Jacobi (fp64), sign rule, record
//   extent_kernel per chunk: min / max of (p - c).e_k through ordered-integer atomics
//   obb_kernel    per (frame, label): OBB centre and half extents
//
// Determinism: every floating-point sum has a fixed order — a wave sums its lanes with a fixed DPP tree (lanes outside
// the object contribute +0.0), a wave adds its own iterations in program order into an LDS row it alone owns, a block
// combines its four waves in wave order, and the reduce / moments kernels add the chunks in chunk order.  No float
// atomics: the only atomics are integer adds and max over order-preserving integer encodings (min = max of the
// complement).  A frame's chunks and partials do not depend on the other frames of the batch, so frame b's outputs are
// the same bits alone or in a batch.
#include "fixed_order.h"
#include "labelmap.h"

#include <limits.h>
#include <math.h>

namespace uoc {
namespace {

constexpr int WAVES = 4;            // waves per block
constexpr int SUB = 1024;           // pixels per wave: a wave owns a contiguous sub-chunk (16 iterations of 64 pixels)
constexpr int CHUNK = WAVES * SUB;  // pixels per block
constexpr int NST = 12;             // integer statistics per (frame, label), see ST_*
constexpr int MAX_ATTR = UOC_OBJECTS_MAX_ATTR;

// Integer statistics: all "max" accumulators (or a count) so that zero is the neutral value of a zeroed buffer.
enum { ST_PIX = 0, ST_X1 = 1, ST_WX = 2, ST_Y1 = 3, ST_HY = 4, ST_MAX = 5, ST_MIN = 8 };
//   ST_X1 = max(x + 1), ST_WX = max(W - x), ST_Y1 = max(y + 1), ST_HY = max(H - y)
//   ST_MAX + k = max(key(p_k)), ST_MIN + k = max(~key(p_k))   over the valid points

__device__ __forceinline__ unsigned fkey(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float fdecode(unsigned k) {
  return __uint_as_float(k ^ ((k & 0x80000000u) ? 0x80000000u : 0xffffffffu));
}
struct Pix {
  int l;       // object id, or -1 for background / out of range
  bool valid;  // valid point
  float x, y, z;
};
__device__ __forceinline__ Pix load_pix(const int *__restrict__ L, const float *__restrict__ X, int n, int p) {
  Pix q{-1, false, 0.f, 0.f, 0.f};
  if (p < n) {
    q.l = obj_key(L[p]);
    if (q.l >= 0) {
      q.x = X[p];
      q.y = X[(size_t)n + p];
      q.z = X[2 * (size_t)n + p];
      q.valid = isfinite(q.x) && isfinite(q.y) && isfinite(q.z) && q.z > 0.f;
    }
  }
  return q;
}

// Workspace layout (uoc_objects_workspace_bytes).  The zeroed part comes first.
struct Ws {
  unsigned *st;                // [B][NUM_IDS][NST]            zeroed
  unsigned long long *ext;     // [B][NUM_IDS][6]  max key(d_k), max ~key(d_k)   zeroed
  int *wcnt;                   // [B][nch][WAVES][NUM_IDS]     valid counts per wave, then rank bases
  double *psum;                // [B][nch][NUM_IDS][3]
  double *pmom;                // [B][nch][NUM_IDS][6]
  double *cent;                // [B][NUM_IDS][3]
  double *axes;                // [B][NUM_IDS][9]  row-major, column k = e_k
  int *info;                   // [B][NUM_IDS][4]  count, kept, prefix of kept within the frame
  int *ftotal;                 // [B]         kept points of the frame
  size_t zero_bytes, total;
};
Ws carve(void *base, int B, int nch) {
  Ws w;
  Carver cv(base);
  w.st = cv.take<unsigned>((size_t)B * NUM_IDS * NST);
  w.ext = cv.take<unsigned long long>((size_t)B * NUM_IDS * 6);
  w.zero_bytes = cv.total();
  w.wcnt = cv.take<int>((size_t)B * nch * WAVES * NUM_IDS);
  w.psum = cv.take<double>((size_t)B * nch * NUM_IDS * 3);
  w.pmom = cv.take<double>((size_t)B * nch * NUM_IDS * 6);
  w.cent = cv.take<double>((size_t)B * NUM_IDS * 3);
  w.axes = cv.take<double>((size_t)B * NUM_IDS * 9);
  w.info = cv.take<int>((size_t)B * NUM_IDS * 4);
  w.ftotal = cv.take<int>((size_t)B);
  w.total = cv.total();
  return w;
}

// ---- 1. count pass ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void count_kernel(const int *__restrict__ labels, const float *__restrict__ xyz, int H,
                                                    int W, int nch, unsigned *__restrict__ st, int *__restrict__ wcnt,
                                                    double *__restrict__ psum) {
  __shared__ unsigned bst[NUM_IDS][NST];
  __shared__ int wvc[WAVES][NUM_IDS];
  __shared__ double wsum[WAVES][NUM_IDS][3];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c = blockIdx.x, b = blockIdx.y, n = H * W;
  for (int i = tid; i < NUM_IDS * NST; i += 256) (&bst[0][0])[i] = 0u;
  for (int i = tid; i < WAVES * NUM_IDS; i += 256) (&wvc[0][0])[i] = 0;
  for (int i = tid; i < WAVES * NUM_IDS * 3; i += 256) (&wsum[0][0][0])[i] = 0.0;
  __syncthreads();
  const int *L = labels + (size_t)b * n;
  const float *X = xyz + (size_t)b * 3 * n;
  const int p0 = c * CHUNK + w * SUB;
  for (int it = 0; it < SUB / 64; ++it) {
    const int base = p0 + it * 64;
    if (base >= n) break;  // uniform per wave
    const int p = base + lane;
    const Pix q = load_pix(L, X, n, p);
    const int px = p % W, py = p / W;
    const unsigned long long vall = __ballot(q.valid);
    for_each_wave_key(q.l, [&](int id, unsigned long long m, int first) {
      const unsigned long long vm = m & vall;
      const bool g = (m >> lane) & 1ull, gv = (vm >> lane) & 1ull;
      const int last = 63 - __clzll((long long)m);
      const unsigned x1 = wave_max_u(g ? (unsigned)(px + 1) : 0u);
      const unsigned wx = wave_max_u(g ? (unsigned)(W - px) : 0u);
      unsigned kmax[3] = {0u, 0u, 0u}, kmin[3] = {0u, 0u, 0u};
      double s[3] = {0.0, 0.0, 0.0};
      if (vm) {
        const float v[3] = {q.x, q.y, q.z};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          kmax[k] = wave_max_u(gv ? fkey(v[k]) : 0u);
          kmin[k] = wave_max_u(gv ? ~fkey(v[k]) : 0u);
          s[k] = wave_sum_d(gv ? (double)v[k] : 0.0);
        }
      }
      if (lane == 0) {
        atomicAdd(&bst[id][ST_PIX], (unsigned)__popcll(m));
        atomicMax(&bst[id][ST_X1], x1);
        atomicMax(&bst[id][ST_WX], wx);
        atomicMax(&bst[id][ST_Y1], (unsigned)((base + last) / W + 1));
        atomicMax(&bst[id][ST_HY], (unsigned)(H - (base + first) / W));
        if (vm) {
          wvc[w][id] += __popcll(vm);
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            atomicMax(&bst[id][ST_MAX + k], kmax[k]);
            atomicMax(&bst[id][ST_MIN + k], kmin[k]);
            wsum[w][id][k] += s[k];
          }
        }
      }
    });
  }
  __syncthreads();
  unsigned *S = st + (size_t)b * NUM_IDS * NST;
  for (int i = tid; i < NUM_IDS * NST; i += 256) {
    const unsigned v = (&bst[0][0])[i];
    if (v == 0u) continue;
    if (i % NST == ST_PIX)
      atomicAdd(&S[i], v);
    else
      atomicMax(&S[i], v);
  }
  int *WC = wcnt + ((size_t)b * nch + c) * WAVES * NUM_IDS;
  for (int i = tid; i < WAVES * NUM_IDS; i += 256) WC[i] = (&wvc[0][0])[i];
  if (tid < NUM_IDS) {
    double *P = psum + (((size_t)b * nch + c) * NUM_IDS + tid) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) P[k] = ((wsum[0][tid][k] + wsum[1][tid][k]) + wsum[2][tid][k]) + wsum[3][tid][k];
  }
}

// ---- 2. reduce: centroid, rank bases, kept counts -----------------------------------------------------------------
__global__ __launch_bounds__(NUM_IDS) void reduce_kernel(int nch, int max_pts, int *__restrict__ wcnt,
                                                    const double *__restrict__ psum, double *__restrict__ cent,
                                                    int *__restrict__ info, int *__restrict__ ftotal) {
  __shared__ int kept_s[NUM_IDS];
  const int l = threadIdx.x, b = blockIdx.x;
  // One thread walks all chunks of its label; the loops are unrolled so that the loads of several chunks are in flight
  // together (the additions stay in chunk order).
  int cnt = 0;
#pragma unroll 8
  for (int c = 0; c < nch; ++c) {
    int *WC = wcnt + ((size_t)b * nch + c) * WAVES * NUM_IDS + l;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      const int v = WC[w * NUM_IDS];
      WC[w * NUM_IDS] = cnt;  // exclusive scan over (chunk, wave): the rank of the wave's first valid point
      cnt += v;
    }
  }
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll 8
  for (int c = 0; c < nch; ++c) {
    const double *P = psum + (((size_t)b * nch + c) * NUM_IDS + l) * 3;
    s0 += P[0];
    s1 += P[1];
    s2 += P[2];
  }
  double *C = cent + ((size_t)b * NUM_IDS + l) * 3;
  C[0] = cnt ? s0 / cnt : 0.0;
  C[1] = cnt ? s1 / cnt : 0.0;
  C[2] = cnt ? s2 / cnt : 0.0;
  const int kept = (max_pts > 0 && cnt > max_pts) ? max_pts : cnt;
  kept_s[l] = kept;
  __syncthreads();
  if (l == 0) {
    int run = 0;
    for (int i = 0; i < NUM_IDS; ++i) {
      const int k = kept_s[i];
      kept_s[i] = run;
      run += k;
    }
    ftotal[b] = run;
  }
  __syncthreads();
  int *I = info + ((size_t)b * NUM_IDS + l) * 4;
  I[0] = cnt;
  I[1] = kept;
  I[2] = kept_s[l];
  I[3] = 0;
}

__device__ __forceinline__ int frame_base(const int *__restrict__ ftotal, int b) {
  int s = 0;
  for (int i = 0; i < b; ++i) s += ftotal[i];
  return s;
}

// ---- 3. scatter + centred second moments ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void scatter_kernel(const int *__restrict__ labels, const float *__restrict__ xyz,
                                                      const float *__restrict__ attr, int C, int H, int W, int nch,
                                                      int max_pts, const int *__restrict__ wcnt,
                                                      const double *__restrict__ cent, const int *__restrict__ info,
                                                      const int *__restrict__ ftotal, float *__restrict__ pts,
                                                      float *__restrict__ pattr, int *__restrict__ ppix, long capacity,
                                                      double *__restrict__ pmom) {
  __shared__ double cs[NUM_IDS][3];
  __shared__ double wmom[WAVES][NUM_IDS][6];
  __shared__ int wrun[WAVES][NUM_IDS];
  __shared__ int off_s[NUM_IDS], cnt_s[NUM_IDS];
  __shared__ int fb_s;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c = blockIdx.x, b = blockIdx.y, n = H * W;
  if (tid == 0) fb_s = frame_base(ftotal, b);
  for (int i = tid; i < NUM_IDS * 3; i += 256) (&cs[0][0])[i] = cent[(size_t)b * NUM_IDS * 3 + i];
  for (int i = tid; i < WAVES * NUM_IDS * 6; i += 256) (&wmom[0][0][0])[i] = 0.0;
  for (int i = tid; i < WAVES * NUM_IDS; i += 256) (&wrun[0][0])[i] = wcnt[((size_t)b * nch + c) * WAVES * NUM_IDS + i];
  __syncthreads();
  if (tid < NUM_IDS) {
    const int *I = info + ((size_t)b * NUM_IDS + tid) * 4;
    cnt_s[tid] = I[0];
    off_s[tid] = fb_s + I[2];
  }
  __syncthreads();
  const int *L = labels + (size_t)b * n;
  const float *X = xyz + (size_t)b * 3 * n;
  const float *A = attr ? attr + (size_t)b * C * n : nullptr;
  const int p0 = c * CHUNK + w * SUB;
  for (int it = 0; it < SUB / 64; ++it) {
    const int base = p0 + it * 64;
    if (base >= n) break;
    const int p = base + lane;
    const Pix q = load_pix(L, X, n, p);
    // only valid points are ranked, written and moment-summed
    for_each_wave_key(q.valid ? q.l : -1, [&](int id, unsigned long long vm, int) {
      const bool gv = (vm >> lane) & 1ull;
      const int r0 = wrun[w][id];
      if (gv && pts) {
        const long long r = r0 + lane_rank(vm), cnt = cnt_s[id];
        long long j = r;
        bool keep = true;
        if (max_pts > 0 && cnt > max_pts) {  // kept ranks floor(j*cnt/M), j = 0..M-1
          j = (r * max_pts + cnt - 1) / cnt;
          keep = j < max_pts && (j * cnt) / max_pts == r;
        }
        const long long pos = off_s[id] + j;
        if (keep && pos < capacity) {
          pts[pos * 3 + 0] = q.x;
          pts[pos * 3 + 1] = q.y;
          pts[pos * 3 + 2] = q.z;
          if (pattr)
            for (int k = 0; k < C; ++k) pattr[pos * C + k] = A[(size_t)k * n + p];
          if (ppix) ppix[pos] = p;
        }
      }
      const double dx = gv ? (double)q.x - cs[id][0] : 0.0;
      const double dy = gv ? (double)q.y - cs[id][1] : 0.0;
      const double dz = gv ? (double)q.z - cs[id][2] : 0.0;
      const double m0 = wave_sum_d(dx * dx), m1 = wave_sum_d(dx * dy), m2 = wave_sum_d(dx * dz);
      const double m3 = wave_sum_d(dy * dy), m4 = wave_sum_d(dy * dz), m5 = wave_sum_d(dz * dz);
      if (lane == 0) {
        wrun[w][id] = r0 + __popcll(vm);
        double *M = wmom[w][id];
        M[0] += m0;
        M[1] += m1;
        M[2] += m2;
        M[3] += m3;
        M[4] += m4;
        M[5] += m5;
      }
    });
  }
  __syncthreads();
  for (int i = tid; i < NUM_IDS * 6; i += 256) {
    const int l = i / 6, k = i - l * 6;
    pmom[((size_t)b * nch + c) * NUM_IDS * 6 + i] = ((wmom[0][l][k] + wmom[1][l][k]) + wmom[2][l][k]) + wmom[3][l][k];
  }
}

// ---- 4. covariance, eigen-decomposition, records ----------------------------------------------------------------------
__global__ __launch_bounds__(NUM_IDS) void moments_kernel(int B, int H, int W, int nch, const unsigned *__restrict__ st,
                                                     const double *__restrict__ pmom, const double *__restrict__ cent,
                                                     const int *__restrict__ info, const int *__restrict__ ftotal,
                                                     double *__restrict__ axes_out, uoc_object *__restrict__ objs,
                                                     int *__restrict__ total) {
  const int l = threadIdx.x, b = blockIdx.x;
  const unsigned *S = st + ((size_t)b * NUM_IDS + l) * NST;
  const int *I = info + ((size_t)b * NUM_IDS + l) * 4;
  const int cnt = I[0];
  uoc_object &o = objs[(size_t)b * NUM_IDS + l];
  o.pixels = (int)S[ST_PIX];
  o.count = cnt;
  o.box[0] = o.pixels ? W - (int)S[ST_WX] : -1;
  o.box[1] = o.pixels ? H - (int)S[ST_HY] : -1;
  o.box[2] = o.pixels ? (int)S[ST_X1] - 1 : -1;
  o.box[3] = o.pixels ? (int)S[ST_Y1] - 1 : -1;
  o.offset = frame_base(ftotal, b) + I[2];
  o.kept = I[1];
  double m[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 8
  for (int c = 0; c < nch; ++c) {  // chunk order; unrolled so that several chunks' loads are in flight
    const double *P = pmom + (((size_t)b * nch + c) * NUM_IDS + l) * 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) m[k] += P[k];
  }
  const double *C = cent + ((size_t)b * NUM_IDS + l) * 3;
  double *AX = axes_out + ((size_t)b * NUM_IDS + l) * 9;
  for (int k = 0; k < 3; ++k) o.obb_center[k] = o.obb_half[k] = 0.f;   // obb_kernel fills them
  if (cnt > 0) {
    for (int k = 0; k < 6; ++k) m[k] /= cnt;
    double a[3][3] = {{m[0], m[1], m[2]}, {m[1], m[3], m[4]}, {m[2], m[4], m[5]}}, v[3][3];
    jacobi3(a, v);
    double lam[3], vec[3][3];
    sort_eig3(a, v, lam, vec);
    double e0[3], e1[3], e2[3];
    for (int i = 0; i < 3; ++i) {
      e0[i] = vec[0][i];
      e1[i] = vec[1][i];
    }
    sign_rule(e0);
    sign_rule(e1);
    e2[0] = e0[1] * e1[2] - e0[2] * e1[1];
    e2[1] = e0[2] * e1[0] - e0[0] * e1[2];
    e2[2] = e0[0] * e1[1] - e0[1] * e1[0];
    for (int i = 0; i < 3; ++i) {
      AX[i * 3 + 0] = e0[i];
      AX[i * 3 + 1] = e1[i];
      AX[i * 3 + 2] = e2[i];
      o.axes[i * 3 + 0] = (float)e0[i];
      o.axes[i * 3 + 1] = (float)e1[i];
      o.axes[i * 3 + 2] = (float)e2[i];
      o.eig[i] = (float)fmax(lam[i], 0.0);  // eigenvalues of a covariance: a rank-deficient one can leave -1e-20
      o.centroid[i] = (float)C[i];
      o.aabb_max[i] = fdecode(S[ST_MAX + i]);
      o.aabb_min[i] = fdecode(~S[ST_MIN + i]);
    }
    for (int k = 0; k < 6; ++k) o.cov[k] = (float)m[k];
  } else {
    for (int i = 0; i < 9; ++i) AX[i] = 0.0, o.axes[i] = 0.f;
    for (int i = 0; i < 3; ++i) o.eig[i] = o.centroid[i] = o.aabb_min[i] = o.aabb_max[i] = 0.f;
    for (int k = 0; k < 6; ++k) o.cov[k] = 0.f;
  }
  if (b == 0 && l == 0) *total = frame_base(ftotal, B);
}

// ---- 5. extents along the axes -----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void extent_kernel(const int *__restrict__ labels, const float *__restrict__ xyz, int H,
                                                     int W, const double *__restrict__ cent,
                                                     const double *__restrict__ axes,
                                                     unsigned long long *__restrict__ ext) {
  __shared__ double cs[NUM_IDS][3];
  __shared__ double ax[NUM_IDS][9];
  __shared__ unsigned long long bext[NUM_IDS][6];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c = blockIdx.x, b = blockIdx.y, n = H * W;
  for (int i = tid; i < NUM_IDS * 3; i += 256) (&cs[0][0])[i] = cent[(size_t)b * NUM_IDS * 3 + i];
  for (int i = tid; i < NUM_IDS * 9; i += 256) (&ax[0][0])[i] = axes[(size_t)b * NUM_IDS * 9 + i];
  for (int i = tid; i < NUM_IDS * 6; i += 256) (&bext[0][0])[i] = 0ull;
  __syncthreads();
  const int *L = labels + (size_t)b * n;
  const float *X = xyz + (size_t)b * 3 * n;
  const int p0 = c * CHUNK + w * SUB;
  for (int it = 0; it < SUB / 64; ++it) {
    const int base = p0 + it * 64;
    if (base >= n) break;
    const Pix q = load_pix(L, X, n, base + lane);
    for_each_wave_key(q.valid ? q.l : -1, [&](int id, unsigned long long vm, int) {
      const bool gv = (vm >> lane) & 1ull;
      const double dx = (double)q.x - cs[id][0], dy = (double)q.y - cs[id][1], dz = (double)q.z - cs[id][2];
      double hi[3], lo[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double d = dx * ax[id][k] + dy * ax[id][3 + k] + dz * ax[id][6 + k];
        hi[k] = wave_max_d(gv ? d : -INFINITY);
        lo[k] = wave_max_d(gv ? -d : -INFINITY);
      }
      if (lane == 0)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          atomicMax(&bext[id][k], dkey(hi[k]));
          atomicMax(&bext[id][3 + k], dkey(lo[k]));
        }
    });
  }
  __syncthreads();
  unsigned long long *E = ext + (size_t)b * NUM_IDS * 6;
  for (int i = tid; i < NUM_IDS * 6; i += 256) {
    const unsigned long long v = (&bext[0][0])[i];
    if (v) atomicMax(&E[i], v);
  }
}

__global__ __launch_bounds__(NUM_IDS) void obb_kernel(const double *__restrict__ cent, const double *__restrict__ axes,
                                                 const unsigned long long *__restrict__ ext, uoc_object *__restrict__ objs) {
  const int l = threadIdx.x, b = blockIdx.x;
  uoc_object *o = objs + (size_t)b * NUM_IDS + l;
  if (o->count <= 0) return;
  const double *C = cent + ((size_t)b * NUM_IDS + l) * 3, *A = axes + ((size_t)b * NUM_IDS + l) * 9;
  const unsigned long long *E = ext + ((size_t)b * NUM_IDS + l) * 6;
  double mid[3];
  for (int k = 0; k < 3; ++k) {
    const double hi = ddecode(E[k]), lo = -ddecode(E[3 + k]);
    mid[k] = 0.5 * (lo + hi);
    o->obb_half[k] = (float)(0.5 * (hi - lo));
  }
  for (int i = 0; i < 3; ++i)
    o->obb_center[i] = (float)(C[i] + ((A[i * 3 + 0] * mid[0] + A[i * 3 + 1] * mid[1]) + A[i * 3 + 2] * mid[2]));
}

}  // namespace
}  // namespace uoc

using namespace uoc;

extern "C" {

size_t uoc_objects_workspace_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0 || (long long)H * W > INT_MAX) return 0;
  const int nch = (int)(((long long)H * W + CHUNK - 1) / CHUNK);
  return carve(nullptr, B, nch).total;
}

int uoc_objects(const int32_t *d_labels, const float *d_xyz, const float *d_attr, int attr_ch, int B, int H, int W,
                int max_points_per_object, uoc_object *d_objects, float *d_points, float *d_point_attr,
                int32_t *d_point_pixel, long capacity, int32_t *d_total, void *d_ws, size_t ws_bytes, void *stream) {
  UOC_REQUIRE(d_labels && d_xyz && d_objects && d_total && d_ws, "uoc_objects: null labels / xyz / objects / total / workspace");
  UOC_REQUIRE(B > 0 && H > 0 && W > 0, "uoc_objects: bad shape B=%d H=%d W=%d", B, H, W);
  UOC_REQUIRE((long long)B * H * W <= INT_MAX, "uoc_objects: B*H*W = %lld exceeds int32 indexing", (long long)B * H * W);
  UOC_REQUIRE(attr_ch >= 0 && attr_ch <= MAX_ATTR, "uoc_objects: attr_ch = %d outside [0, %d]", attr_ch, MAX_ATTR);
  UOC_REQUIRE(attr_ch == 0 || d_attr, "uoc_objects: attr_ch = %d with null attributes", attr_ch);
  UOC_REQUIRE(!d_point_attr || (attr_ch > 0 && d_points), "uoc_objects: point attributes need attr_ch > 0 and points");
  UOC_REQUIRE(!d_point_pixel || d_points, "uoc_objects: point pixel indices need points");
  UOC_REQUIRE(capacity >= 0, "uoc_objects: negative capacity");
  const int nch = (H * W + CHUNK - 1) / CHUNK;
  const Ws w = carve(d_ws, B, nch);
  UOC_REQUIRE(ws_bytes >= w.total, "uoc_objects: workspace %zu < %zu bytes", ws_bytes, w.total);
  const int M = max_points_per_object > 0 ? max_points_per_object : 0;
  hipStream_t st = (hipStream_t)stream;
  UOC_HIP_CHECK(hipMemsetAsync(d_ws, 0, w.zero_bytes, st));
  const dim3 grid(nch, B);
  hipLaunchKernelGGL(count_kernel, grid, dim3(256), 0, st, d_labels, d_xyz, H, W, nch, w.st, w.wcnt, w.psum);
  hipLaunchKernelGGL(reduce_kernel, dim3(B), dim3(NUM_IDS), 0, st, nch, M, w.wcnt, w.psum, w.cent, w.info, w.ftotal);
  hipLaunchKernelGGL(scatter_kernel, grid, dim3(256), 0, st, d_labels, d_xyz, d_point_attr ? d_attr : nullptr, attr_ch, H,
                     W, nch, M, w.wcnt, w.cent, w.info, w.ftotal, d_points, d_point_attr, d_point_pixel, capacity, w.pmom);
  hipLaunchKernelGGL(moments_kernel, dim3(B), dim3(NUM_IDS), 0, st, B, H, W, nch, w.st, w.pmom, w.cent, w.info, w.ftotal,
                     w.axes, d_objects, d_total);
  hipLaunchKernelGGL(extent_kernel, grid, dim3(256), 0, st, d_labels, d_xyz, H, W, w.cent, w.axes, w.ext);
  hipLaunchKernelGGL(obb_kernel, dim3(B), dim3(NUM_IDS), 0, st, w.cent, w.axes, w.ext, d_objects);
  UOC_LAUNCH_CHECK();
  return UOC_OK;
}
}
