// Fusion of posed z-depth maps into a truncated signed distance lattice (include/ren_amd.h "tsdf"): per lattice point the sum
// of the truncated, normalised signed distances to the surfaces the views saw, and the number of views that contributed.
//
// tsdf_integrate_kernel: one lattice point per lane in linear index order, so that the 64 lanes of a wave lie on one lattice
//   line along k (they project onto a short segment of every image) and the two stores coalesce.  The views run in ascending
//   order in batches of REN_TSDF_VIEW_BATCH: the 12 floats of each view of a batch are staged in LDS once per workgroup and
//   read from there by every lane at the same address (a broadcast), never per lane through vector memory.  sum and count are
//   read once, carried in registers over all views and written once.  A lane past the lattice takes part in the barriers and
//   does nothing else.
// No atomics, no cross-lane traffic; every operation is float32 and rounded on its own (-ffp-contract=off), the two divisions
// are IEEE.  Every pixel index is formed from floats already compared against [0, W) and [0, H).
#include "ren_common.h"

namespace {

constexpr int TS_THREADS = REN_MESH_THREADS;
constexpr int TS_BATCH = REN_TSDF_VIEW_BATCH;
static_assert(TS_BATCH * 12 <= TS_THREADS, "one lane stages one float of the batch");

struct ts_k5 { float k00, k01, k02, k11, k12; };
struct ts_d3 { double x, y, z; };

__global__ void __launch_bounds__(TS_THREADS) tsdf_integrate_kernel(const float *__restrict__ depth, int32_t V, int32_t H, int32_t W,
                                                                    const float *__restrict__ cams, ts_k5 K, ts_d3 lo, ts_d3 step,
                                                                    int32_t ny, int32_t nz, int32_t n, float trunc, float z_min,
                                                                    float *__restrict__ sum, int32_t *__restrict__ count) {
    __shared__ float cam[TS_BATCH * 12];
    const int32_t p = (int32_t)(blockIdx.x * TS_THREADS + threadIdx.x);             // n <= 2^30: the grid stays below 2^31 lanes
    const bool live = p < n;
    const int32_t k = live ? p % nz : 0, ij = live ? p / nz : 0;
    const int32_t j = ij % ny, i = ij / ny;
    const float x0 = (float)(lo.x + (double)i * step.x), x1 = (float)(lo.y + (double)j * step.y), x2 = (float)(lo.z + (double)k * step.z);
    const float wf = (float)W, hf = (float)H;                                       // exact: both <= 16384
    const int64_t image = (int64_t)H * W;
    float acc = 0.f;
    int32_t cnt = 0;
    if (live) {
        acc = sum[p];
        cnt = count[p];
    }
    for (int32_t v0 = 0; v0 < V; v0 += TS_BATCH) {
        const int32_t nb = min(TS_BATCH, V - v0);
        __syncthreads();                                                            // the previous batch has been read by every lane
        if ((int32_t)threadIdx.x < nb * 12) cam[threadIdx.x] = cams[(int64_t)v0 * 12 + threadIdx.x];
        __syncthreads();
        if (!live) continue;
        for (int32_t b = 0; b < nb; ++b) {
            const float *c = cam + b * 12;
            const float d0 = x0 - c[0], d1 = x1 - c[1], d2 = x2 - c[2];
            const float z = (c[5] * d0 + c[8] * d1) + c[11] * d2;                   // column 2 of R: the optical axis
            if (!(z > z_min)) continue;
            const float q0 = (c[3] * d0 + c[6] * d1) + c[9] * d2;
            const float q1 = (c[4] * d0 + c[7] * d1) + c[10] * d2;
            const float xn = q0 / z, yn = q1 / z;
            const float u = (K.k00 * xn + K.k01 * yn) + K.k02, w = K.k11 * yn + K.k12;
            const float fu = floorf(u + 0.5f), fv = floorf(w + 0.5f);
            if (!(fu >= 0.f && fu < wf && fv >= 0.f && fv < hf)) continue;          // NaN skips
            const float D = depth[(int64_t)(v0 + b) * image + (int64_t)(int32_t)fv * W + (int32_t)fu];
            if (!(D > 0.f)) continue;                                               // NaN, zero and negative: no information
            const float s = D - z;
            if (s < -trunc) continue;                                               // hidden behind the surface this view saw
            acc += s >= trunc ? 1.0f : s / trunc;
            cnt += 1;
        }
    }
    if (live) {
        sum[p] = acc;
        count[p] = cnt;
    }
}

bool ts_misaligned(const void *p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) != 0; }

bool ts_pos_finite(double v) { return v > 0.0 && v <= 1.7976931348623157e308; }     // false for NaN

bool ts_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

}  // namespace

extern "C" int ren_tsdf_integrate(const float *depth, int32_t V, int32_t H, int32_t W, const float *cams, const float *K5,
                                  const double *lo, const double *step, int32_t nx, int32_t ny, int32_t nz, float trunc, float z_min,
                                  float *sum, int32_t *count, void *stream) {
    if (V < 0 || H < 0 || W < 0 || H > REN_TSDF_MAX_IMAGE || W > REN_TSDF_MAX_IMAGE) return REN_ERR_BAD_ARG;
    const int64_t pixels = (int64_t)V * H * W;                                      // < 2^31 * 2^28: no overflow
    if (pixels >= ((int64_t)1 << 31)) return REN_ERR_BAD_ARG;
    if (nx < 2 || ny < 2 || nz < 2 || (int64_t)nx * ny > REN_MESH_MAX_POINTS || (int64_t)nx * ny * nz > REN_MESH_MAX_POINTS)
        return REN_ERR_BAD_ARG;
    if (!ts_pos_finite((double)trunc) || !ts_pos_finite((double)z_min)) return REN_ERR_BAD_ARG;
    if (!K5 || !lo || !step || !sum || !count || (V > 0 && !cams) || (pixels > 0 && !depth)) return REN_ERR_BAD_ARG;
    if (ts_misaligned(depth, 4) || ts_misaligned(cams, 4) || ts_misaligned(K5, 4) || ts_misaligned(lo, 8) || ts_misaligned(step, 8) ||
        ts_misaligned(sum, 4) || ts_misaligned(count, 4))
        return REN_ERR_BAD_ARG;
    for (int a = 0; a < 3; ++a)
        if (!ts_finite(lo[a]) || !ts_pos_finite(step[a])) return REN_ERR_BAD_ARG;
    if (pixels == 0) return REN_OK;                                                 // no view, or views without a pixel: every lane would skip
    const int32_t n = nx * ny * nz;
    const ts_k5 K = {K5[0], K5[1], K5[2], K5[3], K5[4]};
    const ts_d3 l = {lo[0], lo[1], lo[2]}, s = {step[0], step[1], step[2]};
    hipLaunchKernelGGL(tsdf_integrate_kernel, dim3(ren_blocks(n, TS_THREADS)), dim3(TS_THREADS), 0, (hipStream_t)stream, depth, V, H, W,
                       cams, K, l, s, ny, nz, n, trunc, z_min, sum, count);
    REN_CHECK_LAUNCH();
}
