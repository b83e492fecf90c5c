// Exact nearest neighbour of a set of query points among a set of reference points, through a uniform grid (include/ren_amd.h
// "mesh distance"): the minimum of the float32 squared distance and, among equal minima, the smallest reference index.  The
// result is a function of the two point sets alone -- the grid decides only how many candidates a query looks at.
//
// Kernel 1, nn_cells_kernel: one point per lane.  12 B read, the linear cell id (4 B) written.
// Kernel 2, nn_search_kernel: one query per lane.  The references stand grouped by cell as 16-byte records (x, y, z, the bits
//   of the original index): one load per candidate.  Cell ids run with x fastest, so the cells of one (y, z) row of a shell are
//   one contiguous range of records: a row on the shell's y or z face is ONE range [cell_start[first], cell_start[last + 1]),
//   any other row contributes its two end cells.  After the shell at Chebyshev distance r the lane stops when its best squared
//   distance is below ((r - 2^-6) h)^2 rounded as the distance itself is (no record outside the visited block can
//   be nearer, or as near), or when the block covers the grid.  The shell loop is bounded by max(gx, gy, gz), the row loops by
//   the grid; the candidate loop by nr: both ends of every range read from cell_start are clamped into [0, nr] first.
// No LDS, no atomics, no floating-point reduction; every operation is float32 and rounded on its own (-ffp-contract=off).
#include "ren_common.h"

namespace {

constexpr int NN_THREADS = REN_MESH_THREADS;

struct nn_f3 { float x, y, z; };
struct nn_i3 { int32_t x, y, z; };

// cell coordinate of one coordinate: clamp(floor((x - lo) * inv_h), 0, g - 1); NaN lands in cell 0
__device__ __forceinline__ int32_t nn_axis(float x, float lo, float inv_h, int32_t g) {
    const float fl = floorf((x - lo) * inv_h);
    if (!(fl >= 0.f)) return 0;
    if (fl >= (float)g) return g - 1;
    return (int32_t)fl;
}

__global__ void __launch_bounds__(NN_THREADS) nn_cells_kernel(const float *__restrict__ pts, int64_t n, nn_f3 lo, float inv_h, nn_i3 g,
                                                              int32_t *__restrict__ cell) {
    const int64_t i = (int64_t)blockIdx.x * NN_THREADS + threadIdx.x;
    if (i >= n) return;
    const float *p = pts + 3 * i;
    const int32_t cx = nn_axis(p[0], lo.x, inv_h, g.x), cy = nn_axis(p[1], lo.y, inv_h, g.y), cz = nn_axis(p[2], lo.z, inv_h, g.z);
    cell[i] = (cz * g.y + cy) * g.x + cx;                                           // < gx gy gz <= 2^27
}

// the records [cell_start[first], cell_start[last + 1]) against the query; first <= last are cell ids of the grid
__device__ __forceinline__ void nn_range(const float4 *__restrict__ recs, const int32_t *__restrict__ cell_start, int32_t nr,
                                         int32_t first, int32_t last, float qx, float qy, float qz, float &best, int32_t &best_i) {
    int32_t j = cell_start[first], end = cell_start[last + 1];
    j = j < 0 ? 0 : j;                                                              // whatever cell_start holds, j and end stay in [0, nr]
    end = end > nr ? nr : end;
    for (; j < end; ++j) {
        const float4 c = recs[j];
        const float dx = qx - c.x, dy = qy - c.y, dz = qz - c.z;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        const int32_t i = __float_as_int(c.w);
        if (d2 < best || (d2 == best && i < best_i)) {
            best = d2;
            best_i = i;
        }
    }
}

__global__ void __launch_bounds__(NN_THREADS) nn_search_kernel(const float *__restrict__ queries, int64_t nq,
                                                               const float4 *__restrict__ recs, const int32_t *__restrict__ cell_start,
                                                               int32_t nr, nn_f3 lo, float h, float inv_h, nn_i3 g, int32_t r_max,
                                                               float *__restrict__ d2_out, int32_t *__restrict__ idx_out) {
    const int64_t q = (int64_t)blockIdx.x * NN_THREADS + threadIdx.x;
    if (q >= nq) return;
    const float qx = queries[3 * q], qy = queries[3 * q + 1], qz = queries[3 * q + 2];
    const int32_t cx = nn_axis(qx, lo.x, inv_h, g.x), cy = nn_axis(qy, lo.y, inv_h, g.y), cz = nn_axis(qz, lo.z, inv_h, g.z);
    // the block of radius `cover` around the query's cell contains the grid
    const int32_t cover = max(max(max(cx, g.x - 1 - cx), max(cy, g.y - 1 - cy)), max(cz, g.z - 1 - cz));
    float best = INFINITY;
    int32_t best_i = INT32_MAX;
    for (int32_t r = 0; r <= r_max; ++r) {
        const int32_t x0 = max(cx - r, 0), x1 = min(cx + r, g.x - 1);
        const int32_t y0 = max(cy - r, 0), y1 = min(cy + r, g.y - 1);
        const int32_t z0 = max(cz - r, 0), z1 = min(cz + r, g.z - 1);
        for (int32_t z = z0; z <= z1; ++z) {
            const bool z_face = z == cz - r || z == cz + r;
            for (int32_t y = y0; y <= y1; ++y) {
                const int32_t row = (z * g.y + y) * g.x;
                if (z_face || y == cy - r || y == cy + r) {
                    nn_range(recs, cell_start, nr, row + x0, row + x1, qx, qy, qz, best, best_i);
                } else {                                                            // an inner row: r >= 1, its two end cells
                    if (cx - r >= 0) nn_range(recs, cell_start, nr, row + cx - r, row + cx - r, qx, qy, qz, best, best_i);
                    if (cx + r < g.x) nn_range(recs, cell_start, nr, row + cx + r, row + cx + r, qx, qy, qz, best, best_i);
                }
            }
        }
        if (r >= cover) break;
        if (r >= 1) {
            const float b = ((float)r - 0.015625f) * h;                             // (r - 2^-6) h: r - 2^-6 is exact for r <= 512
            if (best < b * b) break;
        }
    }
    d2_out[q] = best;
    idx_out[q] = best_i == INT32_MAX ? -1 : best_i;
}

bool nn_misaligned(const void *p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) != 0; }

bool nn_bad_grid(int32_t gx, int32_t gy, int32_t gz) {
    return gx < 1 || gy < 1 || gz < 1 || gx > REN_NN_MAX_EXTENT || gy > REN_NN_MAX_EXTENT || gz > REN_NN_MAX_EXTENT;
}

bool nn_finite(float v) { return fabsf(v) <= 3.4028234663852886e38f; }             // false for NaN

bool nn_bad_lo(const float *lo) { return !lo || !nn_finite(lo[0]) || !nn_finite(lo[1]) || !nn_finite(lo[2]); }

bool nn_bad_count(int64_t n) { return n < 0 || n > (int64_t)INT32_MAX; }

}  // namespace

extern "C" int ren_nn_cells(const float *pts, int64_t n, const float *lo, float inv_h, int32_t gx, int32_t gy, int32_t gz,
                            int32_t *cell, void *stream) {
    if (nn_bad_grid(gx, gy, gz) || nn_bad_count(n) || nn_bad_lo(lo) || !(inv_h > 0.f) || !nn_finite(inv_h)) return REN_ERR_BAD_ARG;
    if (n > 0 && (!pts || !cell)) return REN_ERR_BAD_ARG;
    if (nn_misaligned(pts, 4) || nn_misaligned(cell, 4)) return REN_ERR_BAD_ARG;
    if (n == 0) return REN_OK;
    const nn_f3 l = {lo[0], lo[1], lo[2]};
    const nn_i3 g = {gx, gy, gz};
    hipLaunchKernelGGL(nn_cells_kernel, dim3(ren_blocks(n, NN_THREADS)), dim3(NN_THREADS), 0, (hipStream_t)stream, pts, n, l, inv_h, g,
                       cell);
    REN_CHECK_LAUNCH();
}

extern "C" int ren_nn_search(const float *queries, int64_t nq, const float *ref_records, const int32_t *cell_start, int64_t nr,
                             const float *lo, float h, float inv_h, int32_t gx, int32_t gy, int32_t gz, float *d2, int32_t *idx,
                             void *stream) {
    if (nn_bad_grid(gx, gy, gz) || nn_bad_count(nq) || nn_bad_count(nr) || nn_bad_lo(lo)) return REN_ERR_BAD_ARG;
    if (!(h >= 1.17549435e-38f) || !nn_finite(h) || !(inv_h > 0.f) || !nn_finite(inv_h)) return REN_ERR_BAD_ARG;
    const double one = (double)h * (double)inv_h;                                   // exact: two 24-bit significands
    if (!(one >= 1.0 - 0x1p-16 && one <= 1.0 + 0x1p-16)) return REN_ERR_BAD_ARG;     // the margin of the stopping rule assumes it
    if (!cell_start || (nr > 0 && !ref_records) || (nq > 0 && (!queries || !d2 || !idx))) return REN_ERR_BAD_ARG;
    if (nn_misaligned(queries, 4) || nn_misaligned(ref_records, 16) || nn_misaligned(cell_start, 4) || nn_misaligned(d2, 4) ||
        nn_misaligned(idx, 4))
        return REN_ERR_BAD_ARG;
    if (nq == 0) return REN_OK;
    const nn_f3 l = {lo[0], lo[1], lo[2]};
    const nn_i3 g = {gx, gy, gz};
    const int32_t r_max = (gx > gy ? (gx > gz ? gx : gz) : (gy > gz ? gy : gz)) - 1;
    hipLaunchKernelGGL(nn_search_kernel, dim3(ren_blocks(nq, NN_THREADS)), dim3(NN_THREADS), 0, (hipStream_t)stream, queries, nq,
                       (const float4 *)ref_records, cell_start, (int32_t)nr, l, h, inv_h, g, r_max, d2, idx);
    REN_CHECK_LAUNCH();
}
