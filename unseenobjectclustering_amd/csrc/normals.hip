// Surface normals: per-pixel normals and object faces (include/uoc_hip.h, uoc_normals).
// From the XYZ planes, the label map and the uoc_plane record of a frame: per pixel an integer normal from box-summed
// differences of the organised cloud, its class against the support plane (up, side, oblique, down), the azimuth bin of a
// side pixel and whether it grazes; per id a table of face counts with the azimuth histogram.  Integers only, except
// the point quantisation (rintf), the seed of the corrected square root and the optional unit normals.
//
// One memset (the face accumulators in the workspace) and two launches:
//   pixel_kernel   grid (tiles of TH x TW pixels, frames), 4 waves.  The block stages q (three 20-bit components in one
//                  64-bit word) and the id byte (bit 7: not valid) of its tile plus a halo of r + s <= 12 in LDS once,
//                  forms the horizontal and the vertical pair of every pixel of the tile plus a halo of s there (three
//                  16-bit differences and id + 1 in one 64-bit word, 0: no pair), then every thread box-sums the pairs
//                  of its two pixels (rows ty and ty + 8): the condition id(a) == id(p) makes the sum depend on the
//                  centre, so it is not separable.  Cross product, shift, class and azimuth follow in registers; d_n
//                  goes out as one int4 per pixel.  The face counts are privatised in LDS (128 x 40 words): a wave
//                  adds once per distinct key of its 64 pixels (ballot + popcount), the block flushes its non-zero
//                  words with integer atomics.  LDS: 56000 bytes, below the 64 KB that need no opt-in.
//   faces_kernel   one block per frame, one thread per id: the accumulators and the fullest bin into a row of d_faces.
//
// The plane record becomes integers by grid.h's frame_from_plane, rule F of the table grid; the classes and the azimuth
// read its N, U and V.
//
// Determinism: integer adds commute, the bin and the peak are maxima with an index tie-break, so no result depends on
// the order in which lanes, waves or blocks arrive.  Nothing of frame b depends on the other frames of the batch.
#include "grid.h"
#include "prof.h"

namespace uoc {
namespace {

constexpr int FW = UOC_NORMALS_FACE_WORDS;
constexpr int MAX_A = UOC_NORMALS_MAX_DIRS;
constexpr int TW = 32, TH = 16, THREADS = 256;
constexpr int MAX_R = 8, MAX_S = 4, MAX_HALO = MAX_R + MAX_S;
constexpr int QP = TW + 2 * MAX_HALO, QR = TH + 2 * MAX_HALO;  // the staged points: pitch and rows
constexpr int PP = TW + 2 * MAX_S, PR = TH + 2 * MAX_S;        // the pairs
constexpr float Q_LIM = 524287.0f;
constexpr int D_LIM = 16383;
constexpr int F_PIXELS = 0, F_NORMAL = 1, F_GRAZING = 6, F_PEAK = 7, F_HIST = 8;  // class c counts in column 1 + c

static_assert(FW == F_HIST + MAX_A, "a row of faces is eight counters and the histogram");
static_assert(THREADS == TW * TH / 2 && THREADS / 64 * 2 * 2 == TH, "a thread owns the pixels (ty, tx) and (ty + 8, tx)");
static_assert((QR * QP + 2 * PR * PP) * 8 + NUM_IDS * FW * 4 + QR * QP <= 65536, "LDS stays below 64 KB");
static_assert((NUM_IDS * FW) % 4 == 0, "the accumulators are cleared and flushed as int4");

struct Dirs {
  int v[MAX_A][2];
};

// Step F of grid.h; what the classes and the azimuth need of the frame.  No plane records: no plane.
__device__ __forceinline__ Frame make_plane(const uoc_plane *__restrict__ planes, int b) {
  Frame f = {};
  if (planes) {
    const uoc_plane p = planes[b];
    f = frame_from_plane(p);
  }
  return f;
}

__device__ __forceinline__ unsigned long long pack_q(int x, int y, int z) {
  return (unsigned long long)(x & 0xFFFFF) | ((unsigned long long)(y & 0xFFFFF) << 20) | ((unsigned long long)(z & 0xFFFFF) << 40);
}
__device__ __forceinline__ void unpack_q(unsigned long long w, int &x, int &y, int &z) {
  x = (int)((long long)(w << 44) >> 44);
  y = (int)((long long)(w << 24) >> 44);
  z = (int)((long long)(w << 4) >> 44);
}

// Rule D for the ends at s_q / s_id indices ia and ib: (id(a) + 1) << 48 | d_z << 32 | d_y << 16 | d_x, or 0.
__device__ __forceinline__ unsigned long long make_pair(const unsigned long long *__restrict__ s_q,
                                                        const unsigned char *__restrict__ s_id, int ia, int ib, int jump16) {
  const int ida = s_id[ia], idb = s_id[ib];
  if (((ida | idb) & 0x80) || ida != idb) return 0ull;
  int ax, ay, az, bx, by, bz;
  unpack_q(s_q[ia], ax, ay, az);
  unpack_q(s_q[ib], bx, by, bz);
  const int dx = bx - ax, dy = by - ay, dz = bz - az;
  if (abs(dx) > D_LIM || abs(dy) > D_LIM || abs(dz) > jump16) return 0ull;
  return ((unsigned long long)(ida + 1) << 48) | ((unsigned long long)(dz & 0xFFFF) << 32) |
         ((unsigned long long)(dy & 0xFFFF) << 16) | (unsigned long long)(dx & 0xFFFF);
}

__device__ __forceinline__ long long iabs(long long v) { return v < 0 ? -v : v; }

__device__ __forceinline__ unsigned long long isqrt64(unsigned long long S) {  // S < 2^62: as plane.hip corrects its root
  unsigned long long r = (unsigned long long)sqrt((double)S);
  while (r * r > S) --r;
  while ((r + 1) * (r + 1) <= S) ++r;
  return r;
}

// ---- 1. pixels ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void pixel_kernel(const float *__restrict__ xyz, const int *__restrict__ labels,
                                                        const uoc_plane *__restrict__ planes, int H, int W, int tiles_x, int r,
                                                        int s, int jump16, int min_pairs, Dirs dirs, int A, long long c_up,
                                                        long long s_side, int4 *__restrict__ out_n, float *__restrict__ unit,
                                                        int *__restrict__ acc) {
  __shared__ unsigned long long s_q[QR * QP];
  __shared__ unsigned long long s_ph[PR * PP], s_pv[PR * PP];
  __shared__ __attribute__((aligned(16))) int s_faces[NUM_IDS * FW];
  __shared__ unsigned char s_id[QR * QP];
  const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.y;
  const int x0 = (int)(blockIdx.x % (unsigned)tiles_x) * TW, y0 = (int)(blockIdx.x / (unsigned)tiles_x) * TH;
  const size_t n = (size_t)H * W;
  const float *X = xyz + (size_t)b * 3 * n;
  const int *L = labels ? labels + (size_t)b * n : nullptr;
  const Frame pl = make_plane(planes, b);
  const int h = r + s, qw = TW + 2 * h, qh = TH + 2 * h;

  for (int i = tid; i < NUM_IDS * FW / 4; i += THREADS) reinterpret_cast<int4 *>(s_faces)[i] = make_int4(0, 0, 0, 0);
  for (int idx = tid; idx < qh * qw; idx += THREADS) {  // rule P for the tile and its halo
    const int i = idx / qw, j = idx - i * qw, y = y0 - h + i, x = x0 - h + j;
    unsigned long long w = 0ull;
    int idb = 0xFF;  // outside the image: not valid
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const size_t p = (size_t)y * W + x;
      const int l = L ? L[p] : 0;
      idb = obj_id(l);
      const float fx = X[p], fy = X[n + p], fz = X[2 * n + p];
      bool ok = isfinite(fx) && isfinite(fy) && isfinite(fz) && fz > 0.f;
      const float rx = rintf(fx * 16000.0f), ry = rintf(fy * 16000.0f), rz = rintf(fz * 16000.0f);
      ok = ok && fabsf(rx) <= Q_LIM && fabsf(ry) <= Q_LIM && fabsf(rz) <= Q_LIM;
      if (ok)
        w = pack_q((int)rx, (int)ry, (int)rz);
      else
        idb |= 0x80;
    }
    s_q[i * QP + j] = w;
    s_id[i * QP + j] = (unsigned char)idb;
  }
  __syncthreads();
  const int pw = TW + 2 * s, ph = TH + 2 * s;
  for (int idx = tid; idx < ph * pw; idx += THREADS) {  // rule D for the tile and a halo of s: pixel m = staged (i + r, j + r)
    const int i = idx / pw, j = idx - i * pw;
    s_ph[i * PP + j] = make_pair(s_q, s_id, (i + r) * QP + j, (i + r) * QP + j + 2 * r, jump16);
    s_pv[i * PP + j] = make_pair(s_q, s_id, i * QP + j + r, (i + 2 * r) * QP + j + r, jump16);
  }
  __syncthreads();

  const int tx = tid & 31, side = 2 * s + 1;
#pragma unroll 1
  for (int half = 0; half < 2; ++half) {  // uniform: every lane takes part in the ballots below
    const int ty = (tid >> 5) + half * (TH / 2), y = y0 + ty, x = x0 + tx;
    const bool inside = y < H && x < W;
    const int qi = (ty + h) * QP + tx + h;
    const int idb = s_id[qi], id = idb & 0x7F;
    const bool valid = inside && !(idb & 0x80);
    int tX[3] = {0, 0, 0}, tY[3] = {0, 0, 0}, nX = 0, nY = 0;
    if (valid) {  // rule T
      const unsigned want = (unsigned)id + 1u;
      for (int i = 0; i < side; ++i) {
        const unsigned long long *rh = s_ph + (ty + i) * PP + tx, *rv = s_pv + (ty + i) * PP + tx;
        for (int j = 0; j < side; ++j) {
          const unsigned long long a = rh[j], c = rv[j];
          const bool ma = (unsigned)(a >> 48) == want, mc = (unsigned)(c >> 48) == want;
          tX[0] += ma ? (int)(short)a : 0;
          tX[1] += ma ? (int)(short)(a >> 16) : 0;
          tX[2] += ma ? (int)(short)(a >> 32) : 0;
          nX += ma;
          tY[0] += mc ? (int)(short)c : 0;
          tY[1] += mc ? (int)(short)(c >> 16) : 0;
          tY[2] += mc ? (int)(short)(c >> 32) : 0;
          nY += mc;
        }
      }
    }
    int4 o = make_int4(0, 0, 0, 0);
    const float nan = __int_as_float(0x7FC00000);
    float un[3] = {nan, nan, nan};
    int k_norm = -1, k_cls = -1, k_graz = -1, k_bin = -1;
    if (valid && nX >= min_pairs && nY >= min_pairs) {  // rule N
      const long long N0 = (long long)tY[1] * tX[2] - (long long)tY[2] * tX[1];
      const long long N1 = (long long)tY[2] * tX[0] - (long long)tY[0] * tX[2];
      const long long N2 = (long long)tY[0] * tX[1] - (long long)tY[1] * tX[0];
      const unsigned long long g = (unsigned long long)max(max(iabs(N0), iabs(N1)), iabs(N2));
      const int k = g ? max(0, 64 - __clzll((long long)g) - 30) : 0;
      const long long n0 = N0 >> k, n1 = N1 >> k, n2 = N2 >> k;
      if (n0 | n1 | n2) {
        int qx, qy, qz;
        unpack_q(s_q[qi], qx, qy, qz);
        const int graz = (n0 * (qx >> 4) + n1 * (qy >> 4) + n2 * (qz >> 4)) >= 0 ? 1 : 0;
        const unsigned long long S = (unsigned long long)(n0 * n0 + n1 * n1 + n2 * n2);
        int cls = 0, bin = 0;
        if (pl.found) {  // rules C and Z; uniform per frame
          const long long c16 = (n0 * pl.N[0] + n1 * pl.N[1] + n2 * pl.N[2]) * 16384;
          const long long Lr = (long long)isqrt64(S);
          if (c16 >= c_up * Lr) {
            cls = UOC_NORMAL_UP;
          } else if (-c16 >= c_up * Lr) {
            cls = UOC_NORMAL_DOWN;
          } else if (iabs(c16) <= s_side * Lr) {
            cls = UOC_NORMAL_SIDE;
            const long long a = n0 * pl.U[0] + n1 * pl.U[1] + n2 * pl.U[2], bq = n0 * pl.V[0] + n1 * pl.V[1] + n2 * pl.V[2];
            long long best = a * dirs.v[0][0] + bq * dirs.v[0][1];
            for (int d = 1; d < A; ++d) {
              const long long sc = a * dirs.v[d][0] + bq * dirs.v[d][1];
              if (sc > best) {
                best = sc;
                bin = d;
              }
            }
            k_bin = id * FW + F_HIST + bin;
          } else {
            cls = UOC_NORMAL_OBLIQUE;
          }
          k_cls = id * FW + 1 + cls;
        }
        o = make_int4((int)n0, (int)n1, (int)n2, cls | (graz << 3) | (bin << 8) | (nX << 16) | (nY << 24));
        k_norm = id * FW + F_NORMAL;
        if (graz) k_graz = id * FW + F_GRAZING;
        if (unit) {
          const double len = sqrt((double)(long long)S);
          un[0] = (float)((double)n0 / len);
          un[1] = (float)((double)n1 / len);
          un[2] = (float)((double)n2 / len);
        }
      }
    }
    if (inside) {
      const size_t p = (size_t)y * W + x;
      out_n[(size_t)b * n + p] = o;
      if (unit) {
        float *Un = unit + (size_t)b * 3 * n + p;
        Un[0] = un[0];
        Un[n] = un[1];
        Un[2 * n] = un[2];
      }
    }
    wave_add_keys(s_faces, inside ? id * FW + F_PIXELS : -1, 1, lane);
    wave_add_keys(s_faces, k_norm, 1, lane);
    wave_add_keys(s_faces, k_cls, 1, lane);
    wave_add_keys(s_faces, k_graz, 1, lane);
    wave_add_keys(s_faces, k_bin, 1, lane);
  }
  __syncthreads();
  int *ACC = acc + (size_t)b * NUM_IDS * FW;
  for (int i = tid; i < NUM_IDS * FW / 4; i += THREADS) {
    const int4 v = reinterpret_cast<const int4 *>(s_faces)[i];
    if (v.x) atomicAdd(&ACC[4 * i + 0], v.x);
    if (v.y) atomicAdd(&ACC[4 * i + 1], v.y);
    if (v.z) atomicAdd(&ACC[4 * i + 2], v.z);
    if (v.w) atomicAdd(&ACC[4 * i + 3], v.w);
  }
}

// ---- 2. the rows of faces ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NUM_IDS) void faces_kernel(const int *__restrict__ acc, int *__restrict__ faces) {
  const size_t row = ((size_t)blockIdx.x * NUM_IDS + threadIdx.x) * FW;
  const int *R = acc + row;
  int *O = faces + row;
  int peak = -1, best = 0;  // side == 0: an empty histogram
  for (int k = 0; k < MAX_A; ++k) {
    const int v = R[F_HIST + k];
    O[F_HIST + k] = v;
    if (v > best) {
      best = v;
      peak = k;
    }
  }
  for (int k = 0; k < F_PEAK; ++k) O[k] = R[k];
  O[F_PEAK] = peak;
}

size_t acc_bytes(int B) { return align_up((size_t)B * NUM_IDS * FW * sizeof(int), 256); }

}  // namespace
}  // namespace uoc

using namespace uoc;

extern "C" {

size_t uoc_normals_workspace_bytes(int B, int H, int W) {
  if (!image_ok(B, H, W)) return 0;
  return acc_bytes(B);
}

int uoc_normals(const float *d_xyz, const int32_t *d_labels, const uoc_plane *d_planes, int B, int H, int W, int step,
                int window, int jump_mm, int min_pairs, const int32_t *h_dirs, int A, int c_up, int s_side, int32_t *d_n,
                float *d_unit, int32_t *d_faces, void *d_ws, size_t ws_bytes, void *stream) {
  UOC_REQUIRE(d_xyz && d_n && d_faces && h_dirs && d_ws, "uoc_normals: null xyz / n / faces / dirs / workspace");
  UOC_REQUIRE(image_ok(B, H, W), "uoc_normals: bad shape B=%d H=%d W=%d (B in 1..65535, H*W below 2^31)", B, H, W);
  UOC_REQUIRE(step >= 1 && step <= MAX_R, "uoc_normals: step = %d outside [1, %d]", step, MAX_R);
  UOC_REQUIRE(window >= 0 && window <= MAX_S, "uoc_normals: window = %d outside [0, %d]", window, MAX_S);
  UOC_REQUIRE(jump_mm >= 1 && jump_mm <= 1000, "uoc_normals: jump_mm = %d outside [1, 1000]", jump_mm);
  UOC_REQUIRE(min_pairs >= 1 && min_pairs <= (2 * window + 1) * (2 * window + 1), "uoc_normals: min_pairs = %d outside [1, %d]",
              min_pairs, (2 * window + 1) * (2 * window + 1));
  UOC_REQUIRE(A >= 1 && A <= MAX_A, "uoc_normals: %d directions outside [1, %d]", A, MAX_A);
  UOC_REQUIRE(c_up >= 0 && c_up <= (1 << 28) && s_side >= 0 && s_side <= (1 << 28),
              "uoc_normals: c_up = %d or s_side = %d outside [0, 2^28]", c_up, s_side);
  UOC_REQUIRE(c_up > s_side, "uoc_normals: c_up = %d is not above s_side = %d", c_up, s_side);
  Dirs dirs;
  for (int k = 0; k < MAX_A; ++k)
    for (int c = 0; c < 2; ++c) dirs.v[k][c] = k < A ? h_dirs[2 * k + c] : 0;
  for (int k = 0; k < A; ++k)
    UOC_REQUIRE(abs(dirs.v[k][0]) <= 16384 && abs(dirs.v[k][1]) <= 16384, "uoc_normals: direction %d = (%d, %d) outside [-16384, 16384]",
                k, dirs.v[k][0], dirs.v[k][1]);
  UOC_REQUIRE(aligned16(d_n), "uoc_normals: n not 16-byte aligned");
  UOC_REQUIRE(ws_bytes >= acc_bytes(B), "uoc_normals: workspace %zu < %zu bytes", ws_bytes, acc_bytes(B));
  UOC_REQUIRE(aligned16(d_ws), "uoc_normals: workspace not 16-byte aligned");
  const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;  // tiles_x * tiles_y <= H * W: an int
  const double n = (double)B * H * W;
  hipStream_t st = (hipStream_t)stream;
  {
    ProfScope prof(KC_NORMALS_PIXELS, st, 0.0, n * (d_labels ? 32.0 : 28.0) + (d_unit ? n * 12.0 : 0.0));
    UOC_HIP_CHECK(hipMemsetAsync(d_ws, 0, acc_bytes(B), st));
    hipLaunchKernelGGL(pixel_kernel, dim3((unsigned)(tiles_x * tiles_y), B), dim3(THREADS), 0, st, d_xyz, d_labels, d_planes, H, W,
                       tiles_x, step, window, 16 * jump_mm, min_pairs, dirs, A, (long long)c_up, (long long)s_side, (int4 *)d_n,
                       d_unit, (int *)d_ws);
  }
  {
    ProfScope prof(KC_NORMALS_FACES, st, 0.0, (double)B * NUM_IDS * FW * 8.0);
    hipLaunchKernelGGL(faces_kernel, dim3(B), dim3(NUM_IDS), 0, st, (const int *)d_ws, d_faces);
  }
  UOC_LAUNCH_CHECK();
  return UOC_OK;
}

}  // extern "C"
