// Evaluation metrics (include/ren_amd.h "evaluation metrics"): SSIM of every (view, channel) plane in one launch.
//
// torchmetrics.functional.ssim as the reference calls it (loss_metric/metric.py:74-81: 11 x 11 Gaussian window, sigma 1.5,
// k1 0.01, k2 0.03, data_range = the target's largest pixel value): reflect padding by 5, filtering, then a 5-pixel crop of
// every border, so the mean runs over the (H - 10) x (W - 10) valid windows only and the padding never reaches it.
//
// Layout: one workgroup of 256 threads (4 waves) per 64 x 64 tile of a plane's valid output region.  The tile's 74 x 74
// input window (5-pixel halo) of pred and target is staged in LDS as float (43 KB).  Lane l of wave w owns output column l
// and the 16 output rows 16w .. 16w + 15: for each of the 26 input rows that feed them it forms the horizontal 11-tap sums
// of the five moments p, t, p^2, t^2, p t in fp64 (consecutive lanes read consecutive words: no bank conflict) and adds them,
// weighted by the vertical tap, into a sliding set of 11 x 5 fp64 accumulators held in registers (145 VGPRs, no scratch:
// tools/kres.py; a fully unrolled 16-row form spilled).  fp64 is what the metric needs: sigma^2 = E[x^2] - mu^2 cancels, and against C2 =
// (0.03 R)^2 an fp32 restatement is off by ~1e-5.  The SSIM map is summed per thread, per wave (shuffles) and per workgroup
// (LDS) in a fixed order; a second launch adds each plane's tile partials in a fixed order and divides by the window count.
// No atomics: repeated calls are bitwise equal.
#include "ren_common.h"

namespace {

constexpr int SSIM_K = 11, SSIM_R = 5;
constexpr int TILE_W = 64, ROWS_PER_WAVE = 16, WAVES = 4, TILE_H = ROWS_PER_WAVE * WAVES;
constexpr int WIN_W = TILE_W + 2 * SSIM_R, WIN_H = TILE_H + 2 * SSIM_R;       // 74 x 74 input window
constexpr int THREADS = REN_WAVE * WAVES;

struct SsimWeights {
    double g[SSIM_K];
};

__device__ __forceinline__ double wave_sum(double v) {
    // butterfly over the 64 lanes; every lane ends with the same total, formed in the same order on every call
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, REN_WAVE);
    return v;
}

__global__ void __launch_bounds__(THREADS) ssim_tile_kernel(const float *__restrict__ pred, const float *__restrict__ target,
                                                            int H, int W, int tiles_x, int tiles_per_plane, SsimWeights wt,
                                                            double C1, double C2, double *__restrict__ partial) {
    __shared__ float sp[WIN_H * WIN_W], st[WIN_H * WIN_W];
    __shared__ double wsum[WAVES];
    const int tid = threadIdx.x, lane = tid & (REN_WAVE - 1), wave = tid >> 6;
    const int64_t plane = blockIdx.x / tiles_per_plane;
    const int tile = blockIdx.x - (int)(plane * tiles_per_plane);
    const int x0 = (tile % tiles_x) * TILE_W, y0 = (tile / tiles_x) * TILE_H;
    const int Hv = H - 2 * SSIM_R, Wv = W - 2 * SSIM_R;
    const float *P = pred + plane * (int64_t)H * W, *T = target + plane * (int64_t)H * W;
    for (int i = tid; i < WIN_H * WIN_W; i += THREADS) {
        const int r = i / WIN_W, c = i - r * WIN_W, gy = y0 + r, gx = x0 + c;
        const bool in = gy < H && gx < W;                    // cells past the image feed only outputs that are masked below
        sp[i] = in ? P[(int64_t)gy * W + gx] : 0.f;
        st[i] = in ? T[(int64_t)gy * W + gx] : 0.f;
    }
    __syncthreads();

    // acc[j]: the output row r - 10 + j of this wave's strip, over the vertical taps seen so far; after input row r the row in
    // acc[0] is complete and leaves, the others move down one slot (static indices: only the loop over r stays rolled)
    double acc[SSIM_K][5];
#pragma unroll
    for (int j = 0; j < SSIM_K; ++j)
#pragma unroll
        for (int m = 0; m < 5; ++m) acc[j][m] = 0.0;
    const int base = wave * ROWS_PER_WAVE * WIN_W + lane;
    const bool col_ok = x0 + lane < Wv;
    const int row0 = y0 + wave * ROWS_PER_WAVE - 2 * SSIM_R;            // output row of acc[0] at input row r: row0 + r
    double s = 0.0;
#pragma unroll 1
    for (int r = 0; r < ROWS_PER_WAVE + 2 * SSIM_R; ++r) {
        const float *rp = sp + base + r * WIN_W, *rt = st + base + r * WIN_W;
        double h0 = 0.0, h1 = 0.0, h2 = 0.0, h3 = 0.0, h4 = 0.0;
#pragma unroll
        for (int k = 0; k < SSIM_K; ++k) {
            const double p = rp[k], t = rt[k];
            const double gp = wt.g[k] * p, gt = wt.g[k] * t;
            h0 += gp;
            h1 += gt;
            h2 = fma(gp, p, h2);
            h3 = fma(gt, t, h3);
            h4 = fma(gp, t, h4);
        }
#pragma unroll
        for (int j = 0; j < SSIM_K; ++j) {
            const double g = wt.g[SSIM_K - 1 - j];
            acc[j][0] = fma(g, h0, acc[j][0]);
            acc[j][1] = fma(g, h1, acc[j][1]);
            acc[j][2] = fma(g, h2, acc[j][2]);
            acc[j][3] = fma(g, h3, acc[j][3]);
            acc[j][4] = fma(g, h4, acc[j][4]);
        }
        const int y = row0 + r;
        if (r >= 2 * SSIM_R && col_ok && y < Hv) {
            const double mp = acc[0][0], mt = acc[0][1];
            const double mpp = mp * mp, mtt = mt * mt, mpt = mp * mt;
            const double vp = acc[0][2] - mpp, vt = acc[0][3] - mtt, cpt = acc[0][4] - mpt;
            s += ((2.0 * mpt + C1) * (2.0 * cpt + C2)) / ((mpp + mtt + C1) * (vp + vt + C2));
        }
#pragma unroll
        for (int j = 0; j < SSIM_K - 1; ++j)
#pragma unroll
            for (int m = 0; m < 5; ++m) acc[j][m] = acc[j + 1][m];
#pragma unroll
        for (int m = 0; m < 5; ++m) acc[SSIM_K - 1][m] = 0.0;
    }
    s = wave_sum(s);
    if (lane == 0) wsum[wave] = s;
    __syncthreads();
    if (tid == 0) partial[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

__global__ void __launch_bounds__(256) ssim_plane_mean_kernel(const double *__restrict__ partial, int tiles_per_plane,
                                                              double inv_windows, double *__restrict__ out) {
    __shared__ double red[256 / REN_WAVE];
    const int tid = threadIdx.x;
    const double *src = partial + (int64_t)blockIdx.x * tiles_per_plane;
    double s = 0.0;
    for (int i = tid; i < tiles_per_plane; i += 256) s += src[i];
    s = wave_sum(s);
    if ((tid & (REN_WAVE - 1)) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) out[blockIdx.x] = (((red[0] + red[1]) + red[2]) + red[3]) * inv_windows;
}

bool ssim_shape_ok(int64_t P, int32_t H, int32_t W) { return P >= 1 && H >= SSIM_K && W >= SSIM_K; }

int64_t ssim_tiles_per_plane(int32_t H, int32_t W) {
    const int64_t tx = (W - 2 * SSIM_R + TILE_W - 1) / TILE_W, ty = (H - 2 * SSIM_R + TILE_H - 1) / TILE_H;
    return tx * ty;
}

}  // namespace

extern "C" int64_t ren_ssim_scratch_doubles(int64_t P, int32_t H, int32_t W) {
    if (!ssim_shape_ok(P, H, W)) return 0;
    return P * ssim_tiles_per_plane(H, W);
}

extern "C" int ren_ssim_planes(const float *pred, const float *target, int64_t P, int32_t H, int32_t W, double data_range,
                               double *out, double *scratch, void *stream) {
    if (!pred || !target || !out || !scratch) return REN_ERR_BAD_ARG;
    if (!ssim_shape_ok(P, H, W)) return REN_ERR_BAD_ARG;                 // no valid window: torchmetrics would return NaN
    if (!(std::isfinite(data_range) && data_range > 0.0)) return REN_ERR_BAD_ARG;
    const int64_t tiles = ssim_tiles_per_plane(H, W);
    if (P * tiles > INT32_MAX) return REN_ERR_UNSUPPORTED;
    SsimWeights wt;                                                      // torchmetrics _gaussian(11, 1.5), normalised
    double sum = 0.0;
    for (int k = 0; k < SSIM_K; ++k) {
        const double d = (k - SSIM_R) / 1.5;
        wt.g[k] = exp(-0.5 * d * d);
        sum += wt.g[k];
    }
    for (int k = 0; k < SSIM_K; ++k) wt.g[k] /= sum;
    const double C1 = (0.01 * data_range) * (0.01 * data_range), C2 = (0.03 * data_range) * (0.03 * data_range);
    const int tiles_x = (W - 2 * SSIM_R + TILE_W - 1) / TILE_W;
    const double inv_windows = 1.0 / ((double)(H - 2 * SSIM_R) * (double)(W - 2 * SSIM_R));
    hipLaunchKernelGGL(ssim_tile_kernel, dim3((unsigned)(P * tiles)), dim3(THREADS), 0, (hipStream_t)stream, pred, target, H, W,
                       tiles_x, (int)tiles, wt, C1, C2, scratch);
    if (hipGetLastError() != hipSuccess) return REN_ERR_LAUNCH;
    hipLaunchKernelGGL(ssim_plane_mean_kernel, dim3((unsigned)P), dim3(256), 0, (hipStream_t)stream, scratch, (int)tiles,
                       inv_windows, out);
    REN_CHECK_LAUNCH();
}
