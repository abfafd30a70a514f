// Label confidence, the glue around uoc_ms_confidence (csrc/meanshift.hip): no reference counterpart, DESIGN.md section 20.
//   uoc_conf_paste    conf_paste_kernel    crop-level values into the frame along the paint plan of uoc_roi_match
//   uoc_conf_objects  conf_objects_kernel  per-id integer summary (pixels, sum, min, weak) of a (label map, value map) pair
//                     + conf_finish_kernel the minimum out of its accumulator form
// Every result is an integer sum, an integer minimum or a copied float: defined exactly, independent of launch order and batch.
#include "labelmap.h"
#include "prof.h"

#include <limits.h>
#include <math.h>

namespace uoc {

constexpr int QONE = 65536;        // the fixed-point unit of a confidence value

// Source index of frame coordinate c (relative to the box start) in a crop of S along an axis of `len` frame pixels: the
// nearest resize of paste_kernel (csrc/roi.hip), the same float operations in the same order.
__device__ __forceinline__ int paste_src_index(int c, int S, int len) {
  int s = (int)floorf((float)c * ((float)S / (float)len));
  if (s > S - 1) s = S - 1;
  return s;
}

// out[p] = value of the crop pixel whose mapped, non-zero label paste_kernel leaves at p: the same walk over the ROIs, last
// in the paint order first.  A pixel that no ROI paints is not written.
__global__ __launch_bounds__(256) void conf_paste_kernel(const float *__restrict__ values_crop,
                                                         const int *__restrict__ labels_crop,
                                                         const uoc_roi_table *__restrict__ table,
                                                         const int *__restrict__ map, const int *__restrict__ order, int K,
                                                         int S, int H, int W, float *__restrict__ out) {
  const int n = H * W, SS = S * S;
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
    const int y = p / W, x = p - y * W;
    for (int j = K - 1; j >= 0; --j) {
      const int k = order[j];
      if ((unsigned)k >= (unsigned)K) continue;   // not a plan of uoc_roi_match: nothing is read out of bounds
      const int x0 = table->box[k][0], y0 = table->box[k][1], x1 = table->box[k][2], y1 = table->box[k][3];
      if (x < x0 || x > x1 || y < y0 || y > y1) continue;
      const int sy = paste_src_index(y - y0, S, y1 - y0 + 1);
      const int sx = paste_src_index(x - x0, S, x1 - x0 + 1);
      const size_t src = (size_t)k * SS + sy * S + sx;
      const int l = labels_crop[src];
      const int v = ((unsigned)l < (unsigned)NUM_IDS) ? map[k * NUM_IDS + l] : 0;
      if (v != 0) {
        out[p] = values_crop[src];
        break;
      }
    }
  }
}

__device__ __forceinline__ int conf_quantise(float c) {
  if (!(c >= 0.0f)) return 0;          // NaN, negative
  if (c >= 1.0f) return QONE - 1;      // the product is >= 65536
  return (int)(c * (float)QONE);       // exact product (a power of two), truncated
}

// stats [B][128][4] int64, zero-filled: (pixels, sum_q, 65536 - min_q as a maximum with 0 = empty, weak).  Equal labels of a
// wave are combined before the LDS atomics (for_each_wave_key of common.h), a block's rows before the
// global ones.
__global__ __launch_bounds__(256) void conf_objects_kernel(const int *__restrict__ labels, const float *__restrict__ conf,
                                                           int n, int weak_q, long long *__restrict__ stats) {
  __shared__ int s_pix[NUM_IDS], s_inv[NUM_IDS], s_weak[NUM_IDS];
  __shared__ unsigned long long s_sum[NUM_IDS];
  const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.y;
  labels += (size_t)b * n;
  conf += (size_t)b * n;
  stats += (size_t)b * NUM_IDS * 4;
  if (tid < NUM_IDS) {
    s_pix[tid] = 0;
    s_inv[tid] = 0;
    s_weak[tid] = 0;
    s_sum[tid] = 0ull;
  }
  __syncthreads();
  for (int base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x) {   // uniform per block
    const int p = base + tid;
    int l = -1, qv = 0;
    if (p < n) {
      l = label_row(labels[p]);
      qv = conf_quantise(conf[p]);
    }
    for_each_wave_key(l, [&](int c, unsigned long long m, int first) {   // per distinct label of the wave
      const bool hit = l == c;
      const unsigned long long mw = __ballot(hit && qv < weak_q);
      const int sm = wave_sum(hit ? qv : 0);            // <= 64 * 65535
      const int inv = wave_max(hit ? QONE - qv : 0);
      if (lane == first) {
        atomicAdd(&s_pix[c], __popcll(m));
        atomicAdd(&s_sum[c], (unsigned long long)sm);
        atomicMax(&s_inv[c], inv);
        if (mw) atomicAdd(&s_weak[c], __popcll(mw));
      }
    });
  }
  __syncthreads();
  if (tid < NUM_IDS && s_pix[tid]) {
    unsigned long long *row = reinterpret_cast<unsigned long long *>(stats) + 4 * tid;
    atomicAdd(row + 0, (unsigned long long)s_pix[tid]);
    atomicAdd(row + 1, s_sum[tid]);
    atomicMax(row + 2, (unsigned long long)s_inv[tid]);
    if (s_weak[tid]) atomicAdd(row + 3, (unsigned long long)s_weak[tid]);
  }
}

__global__ __launch_bounds__(256) void conf_finish_kernel(long long *__restrict__ stats, int rows) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < rows) stats[4 * (size_t)i + 2] = stats[4 * (size_t)i] > 0 ? QONE - stats[4 * (size_t)i + 2] : 0;
}

static int conf_grid(long n) {
  long b = (n + 255) / 256;
  if (b > 1024) b = 1024;
  return b < 1 ? 1 : (int)b;
}

}  // namespace uoc

using namespace uoc;

extern "C" {

int uoc_conf_paste(const float *d_values_crop, const int32_t *d_labels_crop, const uoc_roi_table *d_table,
                   const int32_t *d_plan, int K, int S, int H, int W, float *d_out, void *stream) {
  UOC_REQUIRE(d_values_crop != nullptr, "uoc_conf_paste: d_values_crop is null");
  UOC_REQUIRE(d_labels_crop != nullptr, "uoc_conf_paste: d_labels_crop is null");
  UOC_REQUIRE(d_table != nullptr, "uoc_conf_paste: d_table is null");
  UOC_REQUIRE(d_plan != nullptr, "uoc_conf_paste: d_plan is null");
  UOC_REQUIRE(d_out != nullptr, "uoc_conf_paste: d_out is null");
  UOC_REQUIRE(K >= 1 && K < NUM_IDS, "uoc_conf_paste: K = %d outside [1, %d]", K, NUM_IDS - 1);
  UOC_REQUIRE(S >= 1 && S <= 4096, "uoc_conf_paste: S = %d outside [1, 4096]", S);
  UOC_REQUIRE(H >= 1 && W >= 1 && (long)H * W <= UOC_CONF_MAX_N, "uoc_conf_paste: bad shape H = %d, W = %d (H * W in 1..%d)", H, W,
              UOC_CONF_MAX_N);
  {  // d_out may not lie on anything the kernel reads while it writes
    struct Span { const char *name; const void *p; size_t bytes; };
    const size_t crops = (size_t)K * S * S * 4;
    const Span in[4] = {{"d_values_crop", d_values_crop, crops}, {"d_labels_crop", d_labels_crop, crops},
                        {"d_table", d_table, sizeof(uoc_roi_table)}, {"d_plan", d_plan, ((size_t)K + (size_t)K * NUM_IDS) * 4}};
    const uintptr_t a = (uintptr_t)d_out;
    const size_t n = (size_t)H * W * 4;
    for (const Span &i : in) {
      const uintptr_t b = (uintptr_t)i.p;
      UOC_REQUIRE(a + n <= b || b + i.bytes <= a, "uoc_conf_paste: d_out aliases %s", i.name);
    }
  }
  hipStream_t st = (hipStream_t)stream;
  ProfScope prof(KC_CONF_GLUE, st, 0.0, 16.0 * H * W);
  hipLaunchKernelGGL(conf_paste_kernel, dim3(conf_grid((long)H * W)), dim3(256), 0, st, d_values_crop, d_labels_crop, d_table,
                     d_plan + K, d_plan, K, S, H, W, d_out);
  UOC_LAUNCH_CHECK();
  return UOC_OK;
}

int uoc_conf_objects(const int32_t *d_labels, const float *d_conf, int B, int H, int W, int weak_q, int64_t *d_stats,
                     void *stream) {
  UOC_REQUIRE(d_labels != nullptr, "uoc_conf_objects: d_labels is null");
  UOC_REQUIRE(d_conf != nullptr, "uoc_conf_objects: d_conf is null");
  UOC_REQUIRE(d_stats != nullptr, "uoc_conf_objects: d_stats is null");
  UOC_REQUIRE(B >= 1 && B <= 65535, "uoc_conf_objects: bad shape B = %d (B in 1..65535)", B);
  UOC_REQUIRE(H >= 1 && W >= 1 && (long)H * W <= UOC_CONF_MAX_N, "uoc_conf_objects: bad shape H = %d, W = %d (H * W in 1..%d)", H,
              W, UOC_CONF_MAX_N);
  UOC_REQUIRE(weak_q >= 0 && weak_q <= QONE - 1, "uoc_conf_objects: weak_q = %d outside [0, %d]", weak_q, QONE - 1);
  UOC_REQUIRE(((uintptr_t)d_stats & 7) == 0, "uoc_conf_objects: d_stats is not 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int n = H * W, rows = B * NUM_IDS;
  ProfScope prof(KC_CONF_GLUE, st, 0.0, 8.0 * B * n + 32.0 * rows);
  UOC_HIP_CHECK(hipMemsetAsync(d_stats, 0, (size_t)rows * 4 * sizeof(int64_t), st));
  int gx = conf_grid(n);
  if (gx > 256) gx = 256;     // 4 pixels or more per thread at 480x640: fewer block rows to fold into the table
  hipLaunchKernelGGL(conf_objects_kernel, dim3(gx, B), dim3(256), 0, st, d_labels, d_conf, n, weak_q,
                     reinterpret_cast<long long *>(d_stats));
  hipLaunchKernelGGL(conf_finish_kernel, dim3((rows + 255) / 256), dim3(256), 0, st, reinterpret_cast<long long *>(d_stats), rows);
  UOC_LAUNCH_CHECK();
  return UOC_OK;
}

}  // extern "C"
